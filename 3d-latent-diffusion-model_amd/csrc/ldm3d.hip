// libldm3d.so - host side: launch plans, weight arena and the C ABI declared in include/ldm3d.h.
//
// The reference (sanazkaviani/3d-latent-diffusion-model) builds its networks by instantiating MONAI classes from
// a JSON "_target_" (3d_ldm/utils.py:243-246) and runs them as a tree of nn.Modules.  Here a model is a flat,
// static LAUNCH PLAN over NDHWC bf16 tensors in one caller-owned workspace: channel concat, nearest upsampling,
// zero padding and 1x1 skip convolutions are addressing modes / extra K steps of the conv kernel, the time-
// embedding bias, conv bias and residual add are conv epilogues, and every ResBlock's time projection is one
// batched GEMV.  Plans are cached per input shape; nothing is allocated or synchronised on the step path.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ldm3d.h"
#include "attention.h"
#include "conv_igemm.h"
#include "conv_halo.h"
#include "conv_cube.h"                 // 3^3 convs over volumes of at most 6^3: weights and the whole volume in LDS once
#include "conv_plane.h"                // 3^3 convs over volumes of at most 12^3, unsplit: one output z-plane per workgroup, epilogue in the kernel
#ifdef LDM_EXPERIMENTS
#include "conv_halo_pp.h"                // alternating K steps per wave group, one barrier per six K steps (experiments builds)
#include "conv_halo_rw.h"                // register-fed weights: built, parity-green, slower
#endif
#include "conv_thin.h"
#include "gemm_light.h"
#include "gemm_wg.h"                  // the light GEMM on operand tiles shared in LDS (one source, K = 128 .. 512)
#include "gemm_light_x3.h"
#include "conv_block.h"
#include "conv_wgrad.h"
#include "conv_wgrad_w16.h"            // sixteen-wave form of the weight gradient for the wide-channel convs
#include "conv_wgrad_kw3.h"            // 3^3 stride-1 weight gradient, three kw taps per workgroup over one shared X tile
#include "norm_elem.h"
#include "window.h"                 // sliding-window sampling: window gather / blend / blend + scheduler step
#include "metrics.h"                // 3-D SSIM + PSNR / MSE / MAE / NRMSE of a volume pair in one pass
#include "likelihood.h"             // variational-bound terms of a given latent (get_likelihood), nearest resize of their maps
#include "ensemble.h"               // per-voxel mean / spread of K sampled volumes: Welford update, std map and scalar statistics
#include "warm_start.h"             // warm starts: seek the device sampler to a row, the noised start x = a z0 + s e
#include "repaint.h"                // inpainting: the repaint step family (base rule, known-region merge, jump back) and its two noise streams
#include "loss_weight.h"            // stage-2 objective: per-timestep loss weights, the per-bin loss tracker and the loss-aware timestep draw
#include "fin_gn.h"
#include "f32_path.h"
#include "f32_train.h"

#ifndef CONV_STAGES
#define CONV_STAGES 4     // depth of the conv kernel's LDS ring (prefetch distance = stages - 1 K steps)
#endif

// ================================================================================================ errors
static thread_local char g_err[1024] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return fail(LDM_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define LDM_TRY(x) do { int r_ = (x); if (r_ != 0) return r_; } while (0)


#ifdef LDM_EXPERIMENTS
static int g_block_slots = 0;                                  // ldm_debug_conv_block_slots: tests walk the tile loop on small volumes
#endif
static hipError_t launch_conv_block(const BlockParams& q0, int TH, hipStream_t s) {
    BlockParams q = q0;
    q.td = (q.D + BLK_TD - 1) / BLK_TD; q.th = (q.H + TH - 1) / TH; q.tw = (q.W + BLK_TW - 1) / BLK_TW;
    const long tiles = (long)q.N * q.td * q.th * q.tw;
    static const int dbg = ldm_xknob("LDM_BLOCK_DBG", 0);
    // the tile-loop form (two workgroups per CU walk the tiles, the next tile's first halo copy issued before the epilogue) lives in experiments
    // builds only (EXTRA=-DLDM_EXPERIMENTS, LDM_CONV_BLOCK_PERSIST=1): 280 vs 255 us at 96^3 (AutoencoderKL encode 2.49 vs 2.35 ms).  A static
    // share of 3 or 4 tiles per workgroup loses what the hardware dispatcher gives the one-tile form for free: the next tile goes to whichever CU
    // frees a slot first.
    static const int persist = ldm_xknob("LDM_CONV_BLOCK_PERSIST", 0);
    static int cus_tab[32] = {};
    int dev_ = 0; if (hipGetDevice(&dev_) != hipSuccess || dev_ < 0 || dev_ >= 32) dev_ = 0;
    if (!cus_tab[dev_]) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev_) != hipSuccess) return hipErrorUnknown; cus_tab[dev_] = pr.multiProcessorCount / 8 * 8; if (cus_tab[dev_] < 8) cus_tab[dev_] = 8; }
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);
    if (!attr_set) {
#define BLK_ATTR(...) { hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_block_kernel<__VA_ARGS__>), hipFuncAttributeMaxDynamicSharedMemorySize, BlkGeom<8>::LDS_ALL); if (e != hipSuccess) return e; }
        BLK_ATTR(8, 0, false) BLK_ATTR(4, 0, false)
#ifdef LDM_EXPERIMENTS
        BLK_ATTR(8, 0, true)
#endif
#ifdef LDM_BLOCK_EXPERIMENTS
        BLK_ATTR(8, 1, false) BLK_ATTR(8, 2, false) BLK_ATTR(8, 4, false) BLK_ATTR(8, 3, false) BLK_ATTR(8, 7, false) BLK_ATTR(8, 8, false) BLK_ATTR(8, 15, false)
#endif
#undef BLK_ATTR
        attr_set = true;
    }
    const unsigned grid = (unsigned)tiles;
#ifdef LDM_BLOCK_EXPERIMENTS
#define BLK_DBG(D) if (TH == 8 && dbg == D) { hipLaunchKernelGGL((conv3_block_kernel<8, D, false>), dim3(grid), dim3(256), BlkGeom<8>::LDS_ALL, s, q); return hipGetLastError(); }
    BLK_DBG(1) BLK_DBG(2) BLK_DBG(4) BLK_DBG(3) BLK_DBG(7) BLK_DBG(8) BLK_DBG(15)
#undef BLK_DBG
#endif
    (void)dbg; (void)persist;
#ifdef LDM_EXPERIMENTS
    const long slots = g_block_slots > 0 ? g_block_slots : 2L * cus_tab[dev_];     // two workgroups per CU
    if (TH == 8 && persist && tiles > slots) { hipLaunchKernelGGL((conv3_block_kernel<8, 0, true>), dim3((unsigned)slots), dim3(256), BlkGeom<8>::LDS_ALL, s, q); return hipGetLastError(); }
#endif
    if (TH == 8) hipLaunchKernelGGL((conv3_block_kernel<8, 0, false>), dim3(grid), dim3(256), BlkGeom<8>::LDS_ALL, s, q);
    else hipLaunchKernelGGL((conv3_block_kernel<4, 0, false>), dim3(grid), dim3(256), BlkGeom<4>::LDS_ALL, s, q);
    return hipGetLastError();
}
// CUs of the current device (256 when there is none: the planner also runs on hosts without a GPU, tests/test_abi_and_host.py)
static int device_cus() {
    static int tab[32] = {};
    int d = 0; if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 32) return 256;
    if (!tab[d]) { hipDeviceProp_t pr; tab[d] = (hipGetDeviceProperties(&pr, d) == hipSuccess && pr.multiProcessorCount >= 8) ? pr.multiProcessorCount : 256; }
    return tab[d];
}
static hipError_t launch_conv_block128(const BlockParams& q0, hipStream_t s) {
    BlockParams q = q0;
    q.td = (q.D + BLK_TD - 1) / BLK_TD; q.th = (q.H + 7) / 8; q.tw = (q.W + BLK_TW - 1) / BLK_TW;
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_block128_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Blk128::LDS_ALL);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(conv3_block128_kernel, dim3((unsigned)((long)q.N * q.td * q.th * q.tw)), dim3(512), Blk128::LDS_ALL, s, q);
    return hipGetLastError();
}
static inline int rup(int v, int m) { return (v + m - 1) / m * m; }
static inline size_t rup_sz(size_t v, size_t m) { return (v + m - 1) / m * m; }

static inline uint16_t host_f2bf(float f) {            // round-to-nearest-even, NaN stays NaN
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// ================================================================================================ plan IR
enum BaseId { BASE_NULL = 0, BASE_WS, BASE_W, BASE_IO0, BASE_IO1, BASE_IO2, BASE_IO3, BASE_IO4, BASE_IO5, BASE_W32, BASE_TAPO, BASE_TAPI, BASE_TTAB, BASE_SST, BASE_COUNT };   // TTAB: tabulated time-embedding rows (model-owned), SST: the sampler's device state
struct Ref { int base = BASE_NULL; size_t off = 0; };
static inline Ref ws_ref(size_t off) { Ref r; r.base = BASE_WS; r.off = off; return r; }
static inline Ref w_ref(size_t off) { Ref r; r.base = BASE_W; r.off = off; return r; }
static inline Ref io_ref(int i) { Ref r; r.base = BASE_IO0 + i; r.off = 0; return r; }
// fp32 precision mode: the matrix at byte offset `off` of the bf16 arena lives unrounded at 2 * off of the fp32 arena
static inline Ref w32_ref(size_t off) { Ref r; r.base = BASE_W32; r.off = 2 * off; return r; }

struct Act {                                         // NDHWC bf16 activation living in the workspace
    size_t off = 0; int C = 0; int N = 0, D = 0, H = 0, W = 0; bool valid = false;
    size_t stats_off = 0; bool has_stats = false;   // GroupNorm partials [blocks][C][2] written by the producer
    int stats_nrb = 0;                               // blocks per sample (0: one per 32 rows of the whole tensor)
    int esz = 2;                                     // bytes per element: 2 = bf16, 4 = fp32 (LDM_PREC_FP32 plans)
    bool hl = false;                                 // fp32 plans: the tensor is stored as [rows][hi(C) | lo(C)] bf16 (same bytes), for the 3 x bf16 halo conv
    size_t cs_off = 0; int cs_rows = 0;              // gradient tensors: column-sum partials [N][cs_rows][C][2] left by the GroupNorm backward that wrote it
    size_t bytes() const { return (size_t)N * D * H * W * C * esz; }
    long rows() const { return (long)N * D * H * W; }
};

enum OpKind { OP_PACK, OP_CONV, OP_FINALIZE, OP_GN_STATS, OP_GN_FINALIZE, OP_GN_PREP, OP_GN_APPLY, OP_ATTN, OP_SINUSOID,
              OP_GEMV, OP_VAE_HEADS, OP_GN_FUSED,
              // backward (training plans only)
              OP_WT /* unused */, OP_WT_BATCH, OP_WGRAD, OP_EXPORT /* unused */, OP_EXPORT_BATCH, OP_COLSUM, OP_GNB, OP_ATTN_BWD, OP_ADD, OP_SUMPOOL, OP_LIN_DX, OP_LIN_DW, OP_VAE_HEADS_BWD,
              OP_GEMM_LIGHT,                       // 1x1 convolution with short K (gemm_light.h)
              OP_COLSUM_BATCH,                     // every column-sum finalize of a backward plan in one launch
              OP_IM2COL,                           // fp32 NCDHW inputs -> bf16 patch matrix of the first conv (pack_im2col_kernel)
              // fp32 precision mode (f32_path.h)
              OP_PACK32, OP_CONV32, OP_FIN32, OP_GN_STATS32, OP_GN_APPLY32, OP_ATTN32, OP_GEMV32,
              OP_TAP,                              // debug tap: export an activation as fp32 NCDHW and / or overwrite it (teacher forcing)
              OP_BUCKET, OP_BUCKET_JOIN,           // training plans: a tail range of the flat gradient buffer is final (all-reduce it now) / wait for every bucket
              OP_UPS_SPLIT32,                      // fp32 precision: nearest x2 upsample into the (hi | lo) bf16 split (upsample_split_f32_kernel)
              OP_CONV_THIN,                        // 3^3 conv with Cout <= 4 and fp32 NCDHW output: the networks' last layer (conv_thin.h)
              OP_FIN_GN,                           // split-K finalize + the GroupNorm(+SiLU) that consumes it, one launch (fin_gn.h)
              OP_GEMM_LIGHT32,
              OP_CONV_BLOCK,                       // 3^3 conv with 64 output channels over a large grid, one halo block in LDS per workgroup (conv_block.h)
              OP_TEMB_ROW,                         // denoise-step plans: the time-embedding projections of the sampler's current step, copied from the table (temb_row_kernel)
              OP_DGRAD_THIN_PACK, OP_DGRAD_THIN,   // backward plans that return input gradients: conv_in's weights re-packed / its thin data gradient into the caller's (dx | dcond) (conv_dgrad_thin.h)
              OP_DGRAD_UNPACK };                   // ... or, behind the general data gradient, the NDHWC gradient of the packed input -> the caller's fp32 NCDHW (dx | dcond) (LayoutRec: a, N, c_real, c_stored, DHW, esz)
             //                   // fp32 precision: 1x1 convolution as the light GEMM on fp32 operands split in registers (gemm_light_x3.h)

struct ConvCfg { int wgm, wgn, bk, splitk; int halo = 0, mtps = 0, qps = 0; int slab_lg = 0; int cube = 0; int th = 0, big = 0; int plane = 0; int wg = 0; };   // cube: conv3_cube_kernel (conv_cube.h), splitk = Cin / 64; plane: conv3_plane_kernel (conv_plane.h), splitk 1   // halo: conv3_halo_kernel (126-row tiles); slab_lg: planar split-K slabs (fin_gn.h)
// th: rows of conv3_block_kernel's tile (OP_CONV_BLOCK, 64 channels); big: 64-row tiles of the light GEMMs (OP_GEMM_LIGHT, OP_GEMM_LIGHT32)
// wg: OP_GEMM_LIGHT on gemm_wg_kernel (gemm_wg.h: operand tiles shared in LDS), same tiles and statistics rows; 2: with the GroupNorm of its input in the prologue

// The record of the convolution family: OP_CONV, OP_FINALIZE, OP_FIN_GN (bf16 kernels, decoded by conv_params) and OP_CONV32, OP_FIN32
// (fp32 kernels, decoded by conv32_params).  Builder::conv_rec fills the geometry, the emit site the rest; a finalize holds a copy of
// its conv's record, or one written next to it, and reads the same `partial` slabs.  The small kernels Builder::conv / conv32 pick for
// some shapes read the same record: OP_CONV_THIN (xa, w, bias, out; x3: ca = 2 Cin as below), OP_CONV_BLOCK (64 or 128 = couts channels,
// ConvCfg::th) and OP_GEMM_LIGHT / OP_GEMM_LIGHT32 (k = 1, K = ca + cb, ConvCfg::big).
struct ConvRec {
    Ref xa, xb, w; int ca, cb;                       // k^3 convolution over the channel-concatenated sources (xa | xb)
    Ref x1a, x1b, w1; int c1a, c1b;                  // fused 1x1 skip over (x1a | x1b) at output resolution (bf16 kernels only)
    int N, Din, Hin, Win, Dout, Hout, Wout;          // input extents: those of xa, before the optional x2 upsample
    int k, stride, pad, M;                           // M = N * Dout * Hout * Wout; phase: k = 2
    int couts, cout_pad, cout_real;                  // stored channels (% 32), weight rows, channels written with f32_out
    int nchunk0, nchunk1, mtiles, ntiles;            // K chunks (Cin / BK) of the k^3 part and of the skip; mtiles, ntiles: fp32 kernels only (bf16: conv_params_geom)
    bool ups, exact;                                 // nearest x2 upsample folded into the loader; exact: zero insertion instead
    bool phase;                                      // (upsample -> 3^3 conv) as eight 2^3 convs on the source grid (ConvParams::phase_mode)
    bool x3;                                         // fp32 precision, 3 x bf16 product on the bf16 kernels: xa = the (hi | lo) split, ca = 2 Cin
    bool ep32_ndhwc, ep32_ncdhw;                     // x3 with splitk 1: the conv's own fp32 epilogue (else it leaves raw slabs for OP_FIN32)
    Ref bias, bias2, temb, residual; int temb_stride;
    Ref out; int f32_out;                            // f32_out: fp32 NCDHW with cout_real channels (the networks' last layer)
    Ref partial, stats;                              // split-K slabs (Builder::finish points them at the shared scratch); GroupNorm partials of the output
    int stats_nrb, stats_rows;                       // OP_FIN32: blocks per sample and rows per block of `stats` (fin32_stats)
    Ref gamma, beta, gn_out; int gn_groups, gn_silu, gn_lg; float gn_eps;   // OP_FIN_GN: the GroupNorm(+SiLU) it applies; gn_lg = log2(channels per group)
    Ref gn_stats; int gn_nrb;                        // OP_GEMM_LIGHT with ConvCfg::wg = 2: GroupNorm (gamma, beta, gn_groups, gn_eps) of xa in the prologue, from xa's partial rows
};

// The record of the GroupNorm family: OP_GN_STATS, OP_GN_FINALIZE, OP_GN_PREP, OP_GN_FUSED, OP_GN_APPLY, their fp32 forms OP_GN_STATS32
// and OP_GN_APPLY32, the backward OP_GNB, and OP_COLSUM (column sums of a gradient tensor through the same slab statistics).
// Builder::gn_rec fills the input, the emit site what its kind reads.  OP_GN_APPLY32 is one of three launches: with nrb_a > 0 it folds
// the producers' partials and applies, with nslab > 0 it folds this plan's slabs (`partial`) and applies, else it applies `ab`.
struct GnRec {
    Ref xa, xb; int ca, cb, N, DHW;                  // the input: channel-concatenated (xa | xb), N samples of DHW voxels
    Ref gamma, beta; int groups; float eps; bool silu;   // the normalisation (silu: GroupNorm + SiLU)
    Ref stats_a, stats_b; int nrb_a, nrb_b;          // (sum, sum of squares) partials the producers of xa / xb left, and their row blocks per sample
    Ref partial; int nslab, rows_per_slab;           // slab partial sums in the shared scratch (Builder::finish) or a block of their own; slabs per sample
    Ref ab, mr;                                      // per-(sample, channel) scale / shift and per-(sample, group) mean / rstd; training plans keep both
    Ref out; bool out_hl;                            // the result; out_hl: stored as the (hi | lo) bf16 split (Act::hl)
    int rows_per_block, chunks;                      // one-launch fold + apply forms (OP_GN_FUSED, OP_GN_APPLY32, OP_GNB): rows per block, grid.x
    // OP_GNB
    Ref dy, gsum, dgamma_n, dbeta_n;                 // incoming gradient, per-(sample, group) sums, per-sample dgamma / dbeta rows (N > 1)
    Ref cs; bool leaves_colsums;                     // the fold form also leaves the column sums of (dxa | dxb) per row chunk in `cs` (Act::cs_off)
    Ref acc_a, acc_b, dxa, dxb;                      // gradients already accumulated for xa / xb (optional), the results
    int dgamma_flat, dbeta_flat;                     // element offsets of the two parameter gradients in the flat gradient buffer
    Ref sink;                                        // data-only backward plans: [2][C] floats that take dgamma | dbeta in place of the flat gradient buffer
    bool fp32;                                       // fp32 precision plan (f32_train.h kernels)
    // OP_COLSUM: out[n * out_stride + c] (over_n: summed over the samples) = column sums of xa's first `count` channels
    int count, out_stride; bool over_n;
};

// The record of OP_WGRAD: dw[taps][Cout][dw_ld], columns [dw_ci_off, dw_ci_off + Cin), from dy and ONE source x of the conv's input
struct WgradRec {
    Ref dy, x, dw; int cdy, cx;                      // cdy, cx: stored channels of dy and x
    int Cout, Cin, dw_ld, dw_ci_off;
    int N, Din, Hin, Win, Dout, Hout, Wout;          // x and dy extents
    int ksize, stride, pad, ups, M;                  // the forward conv; M = rows of dy
    int ksplit, rows_total;                          // voxel split: `ksplit` slabs of [taps][rows_total][dw_ld]
    bool fp32;                                       // fp32 precision plan (wgrad_f32_kernel)
};

// The record of the layout kinds: OP_PACK / OP_PACK32 and OP_IM2COL (the caller's fp32 NCDHW tensors (a | b) -> the NDHWC tensor or the
// first conv's patch matrix `dst`), OP_UPS_SPLIT32 (a -> dst) and OP_TAP (a = the activation, dst = its fp32 NCDHW export, b = the
// caller's tensor that overwrites it).  Builder::pack, conv_in_im2col, tap and the two emit sites in Builder::conv32 fill it.
struct LayoutRec {
    Ref a, b, dst;
    int N, c_real, c_stored, D, H, W, DHW;           // c_stored: channels of the NDHWC side (% 32; im2col: the patch row, Kp); D, H, W or DHW
    bool internal;                                   // pack, im2col: `a` is a tensor of the plan's own with c_real channels, not the caller's (x | cond)
    int esz, mode, ups;                              // tap: bytes per element of a, Builder::tap_mode; ups_split32: log2 of the upsample
    bool guided;                                     // pack, im2col of a guided plan ("unet_cfg*"): N = 2 B samples from the caller's B, the first B with the fill value as condition
};

// The record of OP_ATTN, OP_ATTN32 and OP_ATTN_BWD
struct AttnRec {
    Ref qkv, out, lse;                               // lse: per-(sample, head, voxel) log-sum-exp, training plans only
    Ref d_o, delta, dqkv;                            // backward: incoming gradient, rowsum(dO * O) scratch, the result
    int B, N, C, heads, d; float scale;              // N voxels, C = heads * d, scale = 1 / sqrt(d)
    bool x3, fp32;                                   // OP_ATTN32: 3 x bf16 products (inference plans); OP_ATTN_BWD: fp32 precision plan
};

// The record of the time-embedding path: OP_SINUSOID (x = timesteps -> y[B][O]), OP_TEMB_ROW (y[B][O] from the model's table), OP_GEMV /
// OP_GEMV32 (y = act(w x + bias)) and their backward OP_LIN_DX, OP_LIN_DW
struct LinRec {
    Ref w, bias, x, y;
    Ref dy, x_pre, dx, dW, db, part;                 // backward: x_pre = the linear's input before its SiLU; part: dx partial sums [nz][B][I]
    int B, I, O, x_stride, y_stride, dy_stride;      // row strides in elements
    int silu, nz; bool fp32;                         // silu: x = SiLU(x_pre); nz: splits of O in OP_LIN_DX
};

// The record of the element-wise kinds: OP_ADD (out = a + b over n vectors), OP_SUMPOOL (out = 2^3 sum-pool of a[N][D][H][W][C]),
// OP_VAE_HEADS (ml[B][2 L][DHW] -> mu, sigma, z = mu + sigma * noise) and OP_VAE_HEADS_BWD (dz, g_mu, g_sigma -> dy, the gradient of ml)
struct ElemRec {
    Ref a, b, out; int n;                            // add: n vectors of 16 bytes; sum-pool: a -> out
    Ref ml, noise, mu, sigma, z;                     // VAE heads (the backward reads ml and z again)
    Ref dz, g_mu, g_sigma, dy; int c_dz;             // VAE heads backward: c_dz = stored channels of dz, C those of dy
    int N, D, H, W, C, L, DHW;                       // sum-pool: extents of out; VAE heads: L latent channels, DHW voxels
    bool fp32;                                       // fp32 precision plan
};

// The record of the kinds that run a range: OP_COLSUM_BATCH and OP_EXPORT_BATCH (blocks [first, end) of the table's map), OP_BUCKET
// (`count` elements of the flat gradient buffer from `first`), OP_WT_BATCH (the whole table; fp32)
struct RangeRec { int first, end, count; bool fp32; };

struct Op {
    OpKind kind;
    ConvCfg cc;
    ConvRec cv;                                      // the conv family
    GnRec gn;                                        // the GroupNorm family
    WgradRec wg;                                     // OP_WGRAD
    LayoutRec lay;                                   // pack, im2col, tap, upsample split
    AttnRec at;                                      // attention
    LinRec lin;                                      // time embedding
    ElemRec el;                                      // add, sum-pool, VAE heads
    RangeRec rg;                                     // *_BATCH, bucket
};

struct Pool {                                        // plan-time workspace allocator (first fit + coalescing)
    struct Blk { size_t off, size; };
    std::vector<Blk> free_list;
    std::map<size_t, size_t> live;
    size_t top = 0, high = 0;
    size_t alloc(size_t bytes) {
        bytes = rup_sz(bytes, 256);
        for (size_t k = 0; k < free_list.size(); ++k)
            if (free_list[k].size >= bytes) {
                size_t off = free_list[k].off;
                if (free_list[k].size == bytes) free_list.erase(free_list.begin() + k);
                else { free_list[k].off += bytes; free_list[k].size -= bytes; }
                live[off] = bytes;
                return off;
            }
        size_t off = top; top += bytes; high = std::max(high, top); live[off] = bytes;
        return off;
    }
    void release(size_t off) {
        auto it = live.find(off); if (it == live.end()) return;
        Blk b{off, it->second}; live.erase(it);
        free_list.push_back(b);
        std::sort(free_list.begin(), free_list.end(), [](const Blk& a, const Blk& c) { return a.off < c.off; });
        for (size_t k = 0; k + 1 < free_list.size();)
            if (free_list[k].off + free_list[k].size == free_list[k + 1].off) {
                free_list[k].size += free_list[k + 1].size; free_list.erase(free_list.begin() + k + 1);
            } else ++k;
        if (!free_list.empty() && free_list.back().off + free_list.back().size == top) {
            top = free_list.back().off; free_list.pop_back();
        }
    }
};

// Descriptor table of a batched kernel: device copy of the descriptors + (descriptor, local block) per launched block.
struct DevTable {
    void* descs = nullptr; int2* map = nullptr; int nblocks = 0;
    std::vector<char> h_descs, h_map;                // staged at plan-build time (no device needed), uploaded on first use (ready)
    ~DevTable() { if (descs) (void)hipFree(descs); if (map) (void)hipFree(map); }
    template <class D> int upload(const std::vector<D>& d, const std::vector<int2>& m) {
        if (d.empty()) return 0;
        h_descs.assign((const char*)d.data(), (const char*)(d.data() + d.size()));
        h_map.assign((const char*)m.data(), (const char*)(m.data() + m.size()));
        nblocks = (int)m.size();
        return 0;
    }
    int ready() {
        if (descs || h_descs.empty()) return 0;
        if (hipMalloc(&descs, h_descs.size()) != hipSuccess || hipMalloc((void**)&map, h_map.size()) != hipSuccess) return -1;
        if (hipMemcpy(descs, h_descs.data(), h_descs.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
        if (hipMemcpy(map, h_map.data(), h_map.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
        return 0;
    }
};

struct TapInfo { std::string name; int dims[5]; size_t off; };   // dims = B, C, D, H, W; off = element offset in the tap buffers

struct Plan {
    std::vector<Op> ops;
    std::vector<TapInfo> taps; size_t tap_elems = 0;
    size_t ws_bytes = 0;
    size_t bwd_begin = 0;                            // training plans: ops [0, bwd_begin) = forward, the rest = backward
    bool train = false;
    bool fwd_ran = false;                            // "dec_x": ldm_vae_decode_grad_forward has run this plan (its backward is refused before)
    mutable DevTable wt_tab, exp_tab, cs_tab;                // training plans: all weight transposes / gradient exports / column-sum finalizes in one launch each
};

// ================================================================================================ parameters
enum PackKind { PK_CONV_W, PK_VEC_F32, PK_LINEAR_W };
struct ParamDesc {
    std::string name; std::vector<int64_t> shape;
    PackKind kind; size_t dst_off;                   // arena byte offset of the destination matrix / vector
    int k = 1, cout = 0, cin = 0, cout_pad = 0, cin_s = 0, row_off = 0;
    int64_t flat_off = 0;                            // element offset in the flat fp32 gradient buffer (parameter order)
    bool loaded = false;
};

struct ConvW { size_t w_off = 0; size_t b_off = 0; int cout = 0, cout_pad = 0, cin_s = 0, k = 1; bool has = false;
               size_t wp_off = 0;                    // upsample convs: the derived phase weights [8][8][cout_pad][cin_s] (0 = none)
               size_t x3_off = (size_t)-1;           // fp32 precision: [27][cout_pad][hi | lo | hi] bf16 behind the fp32 arena ((size_t)-1 = none)
               size_t x3p_off = (size_t)-1; };       // ... and of the upsample convs: phase weights [8][8][cout_pad][hi | hi | lo]
struct GnW { size_t g_off = 0, b_off = 0; int C = 0; };
struct LinW { size_t w_off = 0, b_off = 0; int in = 0, out = 0; };

// data-parallel gradient exchange overlapped with backward (ldm_model_set_grad_sync): every OP_BUCKET records an event on the launch
// stream, makes the comm stream wait for it and queues the bucket's all-reduce (mean) there; OP_BUCKET_JOIN makes the launch stream
// wait for the last one.  Timing events (issue point on the launch stream, completion on the comm stream) feed ldm_model_grad_sync_trace.
struct ldm_comm;
struct GradSyncState {
    ldm_comm* comm = nullptr; hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;                      // per bucket: issue (launch stream), done (comm stream); [0] = backward start
    size_t used = 0; std::vector<int64_t> elems;
    int wire = 0;                                    // 0 = fp32 on the wire (the reference's DDP), 1 = bf16 (ldm_model_set_grad_wire)
    void* stage = nullptr; size_t stage_bytes = 0;   // bf16 staging slice of the largest bucket seen (comm stream is in order: one suffices)
    int pending = 0;                                 // buckets handed to the comm stream since the last join
};
static int grad_sync_begin(GradSyncState& g, hipStream_t s);
static int grad_sync_bucket(GradSyncState& g, float* buf, int64_t count, hipStream_t s);
static int grad_sync_join(GradSyncState& g, hipStream_t s);
static int grad_sync_idle(GradSyncState& g, hipStream_t s);
// gradient accumulation over micro-batches (ldm_model_set_grad_accum; grad_accum.h): while acc is set, every OP_BUCKET of a training
// backward folds its finished range of flat_grads into acc, and only the last micro-batch of a window exchanges (the acc range)
struct GradAccumState { float* acc = nullptr; int micro = 0, count = 1; };
static int grad_accum_launch(float* acc, const float* g, int64_t n, float scale, int assign, hipStream_t s);
struct ldm_model {
    int type = 0;                                    // 0 = UNet, 1 = VAE
    ldm_unet_cfg ucfg{}; ldm_vae_cfg vcfg{};
    std::vector<ParamDesc> params;
    std::map<std::string, int> pindex;
    size_t arena_bytes = 8192 + 256;                 // first 8 KiB: the zero page (one padded input row, C <= 4096)
    char* arena = nullptr;
    // fp32 precision mode (ldm_model_set_precision): unrounded copies of every matrix, allocated on first use
    int precision = 0; char* arena32 = nullptr;
    int train_cx = -1, train_cc = 0;                 // (x | cond) channels of the last ldm_unet_train_forward: how ldm_unet_train_backward_input splits dx | dcond
    int loaded_count = 0;
    std::map<std::string, ConvW> convs; std::map<std::string, GnW> gns; std::map<std::string, LinW> lins;
    std::map<std::string, std::shared_ptr<Plan>> plans;
    DevTable pack_tab;                               // one-launch re-pack of a flat fp32 parameter buffer
    // HIP-graph replay of the forward plan (ldm_model_set_graph_mode): one hipGraphLaunch instead of ~150 kernel launches
    // per step on the host.  A graph is instantiated per (plan, pointer set) the second time that set is seen.
    int graph_mode = 0;
    // GraphKey: everything a recorded step bakes in by value, as plain data compared with one memcmp.  A key is zero-filled whole
    // (padding included), then set; what a call does not have stays zero.  plan[1]: the ragged last chunk of a windowed step; ptr: x | xw,
    // cond, tbuf, out, workspace, stream, sampler, the latent stepped in place; rt: runtime x / cond channels; sampler_uid, grid_uid: the
    // never-reused ids (a freed handle's address is readily handed out again); sampler_state: the PNDM buffer bound to the sampler;
    // guide: (w, fill) of a guided step, so compared bit for bit; lik: x0, noise, kl_map, terms, total, scratch of a likelihood step.
    struct GraphKey { const Plan* plan[2]; const void* ptr[8]; const void* sampler_state; const void* grid; const void* lik[6];
                      uint64_t sampler_uid, grid_uid; int rt[2]; int chunk; float guide[2]; };
    struct GraphEntry { GraphKey key; int seen; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    hipStream_t cap_stream = nullptr;        // capture happens on a private stream (the caller's may be the null stream, which cannot capture)
    GradSyncState gsync;                     // ldm_model_set_grad_sync
    GradAccumState gaccum;                   // ldm_model_set_grad_accum
    // UNet: stacked time_emb_proj GEMV
    size_t tproj_w_off = 0, tproj_b_off = 0; int tproj_rows = 0; std::map<std::string, int> tproj_row;
    // UNet: the stacked projections tabulated for every step of a sampler's schedule ([n_steps][tproj_rows] fp32; ldm_unet_denoise_step):
    // valid for the schedule `temb_tab_ts` and the precision it was built in, until the next parameter upload
    float* temb_tab = nullptr; size_t temb_tab_cap = 0; std::vector<float> temb_tab_ts; int temb_tab_prec = -1; bool temb_tab_valid = false;

    size_t arena_alloc(size_t bytes) { size_t o = arena_bytes; arena_bytes += rup_sz(bytes, 256); return o; }
    // weights derived from the packed ones (phase weights of the upsample convs): rebuilt on the stream of the next inference
    // call after any parameter upload
    struct PhaseW { size_t w_off, wp_off; int cout_pad, cin_s; };
    std::vector<PhaseW> phase_ws; bool derived_dirty = true;
    // fp32 precision: bf16 (hi | lo | hi) weights of the 3^3 convs for the 3 x bf16 halo conv, derived from the fp32 arena; they live
    // behind it (arena32 = [2 * arena_bytes fp32 twins][x3_bytes])
    struct X3W { size_t w_off, x3_off; long rows; int cin_s; };
    std::vector<X3W> x3_ws; size_t x3_bytes = 0;
    struct X3PW { size_t w_off, x3p_off; int cout_pad, cin_s; };
    std::vector<X3PW> x3p_ws;
    struct Im2colW { size_t w_off, wi_off; int cout_pad, cin_s, cin, Kp; };     // first convs run as im2col + GEMM (inference plans)
    std::vector<Im2colW> im2col_ws;
    static int im2col_k(int cin) { const int k = 27 * cin; return k <= 96 ? rup(k, 32) : rup(k, 128); }
    // registers <name>.im2col: a 1x1 "conv" over the patch matrix whose weights are derived from <name>'s packed 3^3 weights
    void reg_im2col(const std::string& name, int cin) {
        if (cin > 9) return;
        const ConvW& c3 = convs.at(name);
        ConvW c = c3; c.k = 1; c.cin_s = im2col_k(cin); c.wp_off = 0;
        c.w_off = arena_alloc((size_t)c.cout_pad * c.cin_s * 2);
        im2col_ws.push_back(Im2colW{c3.w_off, c.w_off, c3.cout_pad, c3.cin_s, cin, c.cin_s});
        convs[name + ".im2col"] = c;
    }
    int64_t flat_total = 0;
    void add_param(const ParamDesc& d) {
        pindex[d.name] = (int)params.size(); params.push_back(d);
        ParamDesc& q = params.back(); q.flat_off = flat_total;
        int64_t n = 1; for (auto v : q.shape) n *= v;
        flat_total += n;
    }

    // conv registered under MONAI's Convolution wrapper: <name>.conv.{weight,bias}; several logical convs may
    // share one destination matrix (fused q|k|v, mu|log_sigma) through row_off.
    ConvW reg_conv_into(const std::string& pname, ConvW dst, int cin, int cout, int k, int row_off, bool lin_names) {
        ParamDesc w; w.name = pname + (lin_names ? ".weight" : ".conv.weight");
        if (k == 1 && lin_names) w.shape = {cout, cin}; else w.shape = {cout, cin, k, k, k};
        w.kind = PK_CONV_W; w.dst_off = dst.w_off; w.k = k; w.cout = cout; w.cin = cin;
        w.cout_pad = dst.cout_pad; w.cin_s = dst.cin_s; w.row_off = row_off;
        add_param(w);
        ParamDesc b; b.name = pname + (lin_names ? ".bias" : ".conv.bias"); b.shape = {cout};
        b.kind = PK_VEC_F32; b.dst_off = dst.b_off + (size_t)row_off * 4; b.cout = cout;
        add_param(b);
        return dst;
    }
    ConvW new_conv_slot(int cin_s, int cout_total, int k) {
        ConvW c; c.has = true; c.k = k; c.cout = cout_total; c.cout_pad = rup(cout_total, 64); c.cin_s = cin_s;
        c.w_off = arena_alloc((size_t)k * k * k * c.cout_pad * cin_s * 2);
        c.b_off = arena_alloc((size_t)c.cout_pad * 4);
        return c;
    }
    void reg_x3(ConvW& c) {                          // a 3^3 conv the fp32 inference plans may run on the halo kernel (x3_ws)
        if (c.k != 3 || c.cin_s % 64) return;
        c.x3_off = x3_bytes; x3_bytes += rup_sz((size_t)27 * c.cout_pad * 3 * c.cin_s * 2, 256);
        x3_ws.push_back(X3W{c.w_off, c.x3_off, 27L * c.cout_pad, c.cin_s});
    }
    void reg_conv(const std::string& name, int cin, int cin_s, int cout, int k, bool phase = false) {
        ConvW c = new_conv_slot(cin_s, cout, k);
        if (phase && k == 3) {
            c.wp_off = arena_alloc((size_t)64 * c.cout_pad * cin_s * 2);
            phase_ws.push_back(PhaseW{c.w_off, c.wp_off, c.cout_pad, cin_s});
            if (cin_s % 64 == 0) {
                c.x3p_off = x3_bytes; x3_bytes += rup_sz((size_t)64 * c.cout_pad * 3 * cin_s * 2, 256);
                x3p_ws.push_back(X3PW{c.w_off, c.x3p_off, c.cout_pad, cin_s});
            }
        }
        reg_x3(c);
        reg_conv_into(name, c, cin, cout, k, 0, false);
        convs[name] = c;
    }
    void reg_gn(const std::string& name, int C) {
        GnW g; g.C = C; g.g_off = arena_alloc((size_t)C * 4); g.b_off = arena_alloc((size_t)C * 4);
        ParamDesc w; w.name = name + ".weight"; w.shape = {C}; w.kind = PK_VEC_F32; w.dst_off = g.g_off; w.cout = C; add_param(w);
        ParamDesc b; b.name = name + ".bias"; b.shape = {C}; b.kind = PK_VEC_F32; b.dst_off = g.b_off; b.cout = C; add_param(b);
        gns[name] = g;
    }
    void reg_linear_at(const std::string& name, int in, int out, size_t w_off, size_t b_off) {
        ParamDesc w; w.name = name + ".weight"; w.shape = {out, in}; w.kind = PK_LINEAR_W; w.dst_off = w_off; w.cout = out; w.cin = in; add_param(w);
        ParamDesc b; b.name = name + ".bias"; b.shape = {out}; b.kind = PK_VEC_F32; b.dst_off = b_off; b.cout = out; add_param(b);
    }
    void reg_linear(const std::string& name, int in, int out) {
        LinW l; l.in = in; l.out = out; l.w_off = arena_alloc((size_t)in * out * 2); l.b_off = arena_alloc((size_t)out * 4);
        reg_linear_at(name, in, out, l.w_off, l.b_off);
        lins[name] = l;
    }
    void reg_attn(const std::string& p, int C) {       // SpatialAttentionBlock: norm + fused q|k|v + out_proj
        reg_gn(p + ".norm", C);
        ConvW qkv = new_conv_slot(C, 3 * C, 1);
        reg_conv_into(p + ".attn.to_q", qkv, C, C, 1, 0, true);
        reg_conv_into(p + ".attn.to_k", qkv, C, C, 1, C, true);
        reg_conv_into(p + ".attn.to_v", qkv, C, C, 1, 2 * C, true);
        convs[p + ".attn.qkv"] = qkv;
        ConvW o = new_conv_slot(C, C, 1);
        reg_conv_into(p + ".attn.out_proj", o, C, C, 1, 0, true);
        convs[p + ".attn.out_proj"] = o;
    }
};

// ================================================================================================ builder
static int wgrad_ksplit(long M, int taps, int cout, int cin, bool hp = false, int stride = 1, int ups = 0);
static void conv32_cfg(long M, int cout_pad, int steps, bool x3, int* bn_out, int* sk_out);
static int fin32_stats_blocks(int N, int dhwo, int couts, int* rows);

// ---- launch geometry of the bf16 conv / GroupNorm kernels and of the training plans, shared by the Builder and the ldm_op_* entries that
//      launch the same kernels (the conv configuration itself: Builder::pick_cfg, next to choose_cfg)
// Voxel slabs of the per-(sample, channel) partial sums (gn_stats_kernel, gn_bwd_stats_kernel and their fp32 forms; gn_stats_kernel also as
// the column sums of Builder::emit_colsum): 256 threads over C / vec channel vectors, at most max_slabs / N slabs per sample, none empty.
static void gn_slabs(int N, int C, int DHW, int vec, int max_slabs, int* nslab, int* rps) {
    const int rows_par = std::max(1, 256 / std::max(1, C / vec));
    const int ns = std::min((DHW + rows_par - 1) / rows_par, std::max(1, max_slabs / N));
    *rps = (DHW + ns - 1) / ns;
    *nslab = (DHW + *rps - 1) / *rps;
}
// Row chunks (grid.x) of the one-launch fold + apply kernels, whose grid.y is the 64-channel slices: about `blocks` workgroups in all,
// *rpb = rows per block (a multiple of row_multiple), no chunk empty.
static int gn_row_chunks(int N, int C, int DHW, int blocks, int row_multiple, int* rpb) {
    const int slices = (C + 63) / 64;
    const int chunks = std::max(1, std::min(blocks / (slices * N), (DHW + row_multiple - 1) / row_multiple));
    *rpb = rup((DHW + chunks - 1) / chunks, row_multiple);
    return (DHW + *rpb - 1) / *rpb;
}
// Workgroups of gn_fused_apply_kernel (tuning knob): 512 = two blocks per CU at 24^3 (the apply is VALU-latency bound at one wave per SIMD:
// +0.3 % over the step; 1024: -1 %, every block folds the slabs again)
static int gn_fused_blocks() { static const int v = ldm_xknob("LDM_GN_BLOCKS", 512); return v; }
// Row chunks of gn_bwd_fold_apply_kernel (grid.x): returns the chunk count and *rpb = rows per block (a multiple of 32), or 0 where
// the fold form does not apply (channels per group > 64: the cover exceeds the kernel's LDS; more than 512 partial rows per sample).
static int gnb_fold_chunks(int N, int C, int groups, int DHW, int nslab, int* rpb) {
    if (C / groups > 64 || nslab > 512) return 0;
    return gn_row_chunks(N, C, DHW, 256, 32, rpb);
}
// Output-row slices of linear_bwd_dx_part_kernel (grid.z) for a layer with O outputs.
static int lin_dx_nz(int O) { return std::max(1, std::min(64, O / 64)); }
// Output extent of a k^3 conv over an input edge `in` (taken before the optional x2 upsample); stride 2 with pad 0 is the F.pad(0,1) form
static int conv_out_size(int in, int k, int stride, int pad, int ups) {
    return ((in << ups) + ((stride == 2 && pad == 0 && k == 3) ? 1 : 2 * pad) - k) / stride + 1;
}
// M tiles of a bf16 conv launch: halo tiles and phase-mode tiles (per (sample, parity) of the source grid) never straddle samples
static int conv_mtiles(const ConvRec& c, const ConvCfg& cc) {
    const int bm = 64 * cc.wgm;
    if (cc.halo) return c.N * cc.mtps;
    if (c.phase) return c.N * 8 * (int)(((long)c.Din * c.Hin * c.Win + bm - 1) / bm);
    return (c.M + bm - 1) / bm;
}
// Rows per sample of the GroupNorm partials a split-K finalize leaves (one per 32 output rows); 0 where those straddle samples
static int splitk_stats_rows(int N, int dhw) { return N == 1 ? (dhw + 31) / 32 : dhw % 32 ? 0 : dhw / 32; }
// Rows per sample of the GroupNorm partials of a bf16 conv's output, one per tile of the launch; 0: not available (tiles straddle samples)
static int conv_stats_rows(const ConvRec& c, const ConvCfg& cc) {
    const int dhwo = c.Dout * c.Hout * c.Wout, bm = 64 * cc.wgm;
    if (cc.splitk > 1) return splitk_stats_rows(c.N, dhwo);
    if (cc.plane) return c.Dout;                                             // one row per output plane
    if (cc.halo || c.phase) return conv_mtiles(c, cc) / c.N;
    return c.N == 1 ? (c.M + bm - 1) / bm : dhwo % bm ? 0 : dhwo / bm;
}

struct Builder {
    ldm_model* m; Plan* plan; Pool pool;
    size_t partial_off = 0, partial_bytes = 0;       // shared split-K slab scratch (sized at the end)
    size_t gnpart_off = 0, gnpart_bytes = 0;         // GroupNorm partial sums
    size_t gnab_off = 0, gnab_bytes = 0;             // GroupNorm per-channel scale/shift
    std::vector<size_t> partial_fixups, gnpart_fixups, gnab_fixups;   // op indices whose refs need final offsets
    std::string err;

    Act new_act(int N, int D, int H, int W, int C) {
        Act a; a.N = N; a.D = D; a.H = H; a.W = W; a.C = C; a.valid = true; a.esz = hp ? 4 : 2; a.off = pool.alloc(a.bytes()); return a;
    }
    bool hp = false;                                  // fp32 precision plan (f32_path.h kernels, fp32 activations)
    // debug taps (ldm_*_taps entry points): 0 = none, 1 = export every block output, 2 = export, then overwrite it with the
    // caller's tensor (teacher forcing: the next block sees the reference's input)
    int tap_mode = 0;
    void tap(const std::string& name, Act& h, int c_real) {
        if (!tap_mode) return;
        TapInfo t; t.name = name; t.dims[0] = h.N; t.dims[1] = c_real; t.dims[2] = h.D; t.dims[3] = h.H; t.dims[4] = h.W; t.off = plan->tap_elems;
        plan->tap_elems += (size_t)h.N * c_real * h.D * h.H * h.W;
        Op o{}; o.kind = OP_TAP; LayoutRec& l = o.lay; l.a = ws_ref(h.off);
        l.dst.base = BASE_TAPO; l.dst.off = t.off * 4; l.b.base = BASE_TAPI; l.b.off = t.off * 4;
        l.N = h.N; l.c_real = c_real; l.c_stored = h.C; l.DHW = h.D * h.H * h.W; l.esz = h.esz; l.mode = tap_mode;
        plan->ops.push_back(o);
        plan->taps.push_back(t);
        if (tap_mode == 2 && h.has_stats) { pool.release(h.stats_off); h.has_stats = false; }   // the producer's GroupNorm partials describe the overwritten tensor
    }
    // fp32 NCDHW (src_a | src_b) -> the NDHWC tensor dst, channels past c_real zero.  internal: src_a is a tensor of the plan's own with
    // c_real channels; else the two are the caller's (x | cond), whose channel counts arrive with the call
    void pack(Ref src_a, Ref src_b, const Act& dst, int c_real, bool internal) {
        Op o{}; o.kind = hp ? OP_PACK32 : OP_PACK; LayoutRec& l = o.lay; l.a = src_a; l.b = src_b; l.dst = ws_ref(dst.off);
        l.N = dst.N; l.c_real = c_real; l.c_stored = dst.C; l.DHW = dst.D * dst.H * dst.W; l.internal = internal;
        l.guided = guided && !internal;
        plan->ops.push_back(o);
    }
    void free_act(Act& a) {
        if (train) return;                          // training plans keep every activation for the backward pass
        if (a.valid) { pool.release(a.off); if (a.has_stats) pool.release(a.stats_off); }
        a.valid = false; a.has_stats = false;
    }
    bool train = false, recording = false;
    bool guided = false;                              // classifier-free guidance plan: the caller's (x | cond) are packed twice (LayoutRec::guided)

    // ---- conv ---------------------------------------------------------------------------------------
    struct ConvArgs {
        Act xa, xb;                                   // group-0 sources (xb optional)
        const ConvW* w = nullptr;
        int k = 3, stride = 1, pad = 1, ups = 0;
        int Do = 0, Ho = 0, Wo = 0;
        Act g1a, g1b; const ConvW* w1 = nullptr;     // fused 1x1 skip (optional)
        Ref temb; int temb_stride = 0;               // optional per-sample channel bias
        Act residual;                                // optional
        bool f32_out = false; Ref out_ref; int cout_real = 0;
        bool want_stats = true;                       // also emit the output's GroupNorm partials
        // backward-pass uses of the same kernel (data gradients)
        Ref w_over; bool no_bias = false; int exact = 0;   // weights from the workspace; zero-insertion upsample
        int temb_row = -1;                            // first row of this ResBlock in the stacked time projection
        int f32_tag = 0;                              // which externally supplied gradient an fp32-output conv receives (0 final, 1 VAE heads)
        const GnW* pre_gn = nullptr; int pre_groups = 0, pre_nrb = 0; float pre_eps = 0.f;   // GroupNorm of xa (from its partial rows) in the prologue of gemm_wg_kernel: Builder::attention
    };
    struct Tape {                                    // one differentiable forward op, recorded in training plans
        int kind = 0;                                 // 0 conv, 1 GroupNorm(+SiLU), 2 attention
        ConvArgs c; Act out; bool leaf_input = false;
        const GnW* g = nullptr; Act xa, xb; size_t ab_off = 0, mr_off = 0; int groups = 0; bool silu = false;
        Act qkv, o; size_t lse_off = 0; int head_ch = 64;
    };
    std::vector<Tape> tape;

    static bool halo_enabled() { return ldm_knob("LDM_CONV_HALO", 1) != 0; }
    // LDM_HALO_TALL: 0 = never, 1 = wherever the cost model prefers it, 2 (default) = only for Cout % 128 != 0
    static int tall_mode() { return ldm_xknob("LDM_HALO_TALL", 2); }
    static bool light_enabled() { return ldm_knob("LDM_GEMM_LIGHT", 1) != 0; }
    static bool two_wg_enabled() { return ldm_knob("LDM_IGEMM_2WG", 1) != 0; }
    static bool phase_enabled() { return ldm_knob("LDM_CONV_PHASE", 1) != 0; }
    // halo_n > 0: the conv is eligible for conv3_halo_kernel (3^3, stride 1, pad 1, single source, BK 64); halo_n = N
    // and halo_dhw = voxels per sample (its 126-row tiles never straddle samples).
    // steps = K steps of the 3^3 (or k^3) part; steps1 = extra K steps of a fused 1x1 skip (the halo kernel runs them as a second loop
    // behind the 3^3 one, unsplit convs only)
    static bool halo_skip_enabled() { static const int v = ldm_knob("LDM_HALO_SKIP", 1); return v != 0; }
    static bool halo_skip_split_enabled() { static const int v = ldm_knob("LDM_HALO_SKIP_SPLIT", 1); return v != 0; }   // ... in split-K convs too
    // conv3_cube_kernel (conv_cube.h) for the 3^3 stride-1 convs of volumes up to 6^3 (the UNet's 6^3 level): one workgroup per (sample,
    // 16-cout slice, 64-channel Cin chunk), splitk = Cin / 64.  Same eligibility as the halo kernel plus D, H, W <= 6 and 64-channel skip
    // sources.  LDM_CONV_CUBE=0: those convs go back to conv3_halo_kernel's split-K form.  Read per plan (the operator tests flip it in-process).
    static bool cube_enabled() { return ldm_knob("LDM_CONV_CUBE", 1) != 0; }
    static bool cube_ok(int D, int H, int W, int cin0, int c1a, int c1b, int cout_pad) {
        return cube_enabled() && D >= 1 && H >= 1 && W >= 1 && D <= CUBE_EDGE && H <= CUBE_EDGE && W <= CUBE_EDGE && cin0 % 64 == 0 && cin0 >= 128 &&
               c1a % 64 == 0 && c1b % 64 == 0 && cout_pad % 16 == 0;
    }
    static ConvCfg cube_cfg(int cin0) { ConvCfg c{2, 2, 64, cin0 / 64}; c.cube = 1; return c; }
    // conv3_plane_kernel (conv_plane.h) for the 3^3 stride-1 convs of volumes past the cube kernel's up to 12^3 (the UNet's 12^3 level): one
    // workgroup per (sample, output plane, 16-cout slice) over the whole K range: no split, no slabs, no finalize.  Same eligibility as the
    // cube kernel with every edge <= 12 and one > 6.  LDM_CONV_PLANE=0: those convs go back to conv3_halo_kernel's split-K form;
    // LDM_CONV_PLANE_MAX_CIN: the widest main source it takes.  Its time grows with Cin (11 us per 256 channels: every workgroup takes in
    // 864 * Cin bytes of weights and as many of voxels), the split-K form's hardly does: per op at 12^3, 256 outputs: Cin 256 18.4 vs 26.4 us
    // (halo + finalize), 512 29.5 vs 29.3, 768 40.8 vs 33.2 (profiles/r07_summary.md), so the default admits Cin <= 256.  Read per plan.
    static bool plane_enabled() { return ldm_knob("LDM_CONV_PLANE", 1) != 0; }
    static int plane_max_cin() { return (int)ldm_knob("LDM_CONV_PLANE_MAX_CIN", 256); }
    static bool plane_ok(int D, int H, int W, int cin0, int c1a, int c1b, int cout_pad) {
        return plane_enabled() && D >= 1 && H >= 1 && W >= 1 && D <= PLANE_EDGE && H <= PLANE_EDGE && W <= PLANE_EDGE &&
               (D > CUBE_EDGE || H > CUBE_EDGE || W > CUBE_EDGE) && cin0 % 64 == 0 && cin0 >= 128 && cin0 <= plane_max_cin() &&
               c1a % 64 == 0 && c1b % 64 == 0 && cout_pad % 16 == 0;
    }
    static ConvCfg plane_cfg() { ConvCfg c{2, 2, 64, 1}; c.plane = 1; return c; }
    static ConvCfg choose_cfg(long M, int cout_pad, int steps0, int bk, int halo_n = 0, long halo_dhw = 0, bool halo_only = false, int steps1 = 0) {
        ConvCfg best{2, 2, bk, 1}; double best_t = 1e30;
        const int steps = steps0 + steps1;
        const int rb = bk * 2;
        static const int splits[] = {1, 2, 3, 4, 6, 8, 9, 12, 16, 18, 24, 27, 32, 48, 64};
        for (int wgn = 1; wgn <= 4 && !halo_only; wgn *= 2) {
            const int bn = 64 * wgn, bm = 64 * (4 / wgn);
            if (cout_pad % bn) continue;
            const long tiles = ((M + bm - 1) / bm) * (cout_pad / bn);
            const double c_mfma = (double)bm * bn * bk * 2.0 / 4096.0;           // cycles at the per-CU MFMA peak
            const double c_load = (double)(bm + bn) * rb / 28.0;                 // ~28 B/clk/CU global->LDS
            const double c_step = std::max(c_mfma, c_load) + 60.0;
            for (int sk : splits) {
                if (sk > 1 && steps / sk < 6) break;
                const long nwg = tiles * sk;
                const int sps = (steps + sk - 1) / sk;
                const double rounds = ceil((double)nwg / 256.0);
                double t = rounds * (sps * c_step + 2500.0);
                if (sk > 1) t += 6000.0 + (double)M * cout_pad * 4.0 * sk * 2.0 / 2500.0;   // slab write+read, ~2.5 KB/clk chip
                if (t < best_t) { best_t = t; best = ConvCfg{4 / wgn, wgn, bk, sk}; }
            }
        }
        if (halo_n > 0 && bk == 64 && cout_pad % 128 == 0 && halo_enabled()) {
            const int mtps = (int)((halo_dhw + 125) / 126), Q = steps0 / 3;      // steps0 = 27 * nchunk
            const long tiles = (long)halo_n * mtps * (cout_pad / 128);
            const double c_mfma = 128.0 * 128.0 * 64.0 * 2.0 / 4096.0;
            const double c_load = (128.0 / 3.0 + 128.0) * 128.0 / 28.0;          // the voxel tile is copied once per 3 steps
            const double c_step = std::max(c_mfma, c_load) + 30.0;
            for (int sk : splits) {
                if (sk > 1 && Q / sk < 3) break;
                const int qps = (Q + sk - 1) / sk, skr = (Q + qps - 1) / qps;    // every split non-empty
                const long nwg = tiles * skr;
                const double rounds = ceil((double)nwg / 256.0);
                double t = rounds * (3.0 * qps * c_step + 2500.0 + ((steps1 + skr - 1) / skr) * 1.6 * c_step + (steps1 && skr > 1 ? 800.0 : 0.0));
                if (skr > 1) t += 6000.0 + (double)M * cout_pad * 4.0 * skr * 2.0 / 2500.0;
                if (steps1 && skr > 1 && !halo_skip_split_enabled()) continue;   // the splits share the fused skip's K steps (round 5)
                if (t < best_t) { best_t = t; best = ConvCfg{2, 2, 64, skr}; best.halo = 1; best.mtps = mtps; best.qps = qps; }
            }
        }
        // the tall halo tile (254 voxels x 64 couts, halo = 2): always for Cout % 128 != 0, else where the model says so
        if (halo_n > 0 && bk == 64 && cout_pad % 64 == 0 && halo_enabled() && tall_mode() != 0) {
            const int mtps = (int)((halo_dhw + 253) / 254), Q = steps0 / 3;
            const long tiles = (long)halo_n * mtps * (cout_pad / 64);
            const double c_mfma = 256.0 * 64.0 * 64.0 * 2.0 / 4096.0;
            const double c_load = (256.0 / 3.0 + 64.0) * 128.0 / 28.0;
            const double c_step = std::max(c_mfma, c_load) + 30.0;
            for (int sk : splits) {
                if (sk > 1 && Q / sk < 3) break;
                const int qps = (Q + sk - 1) / sk, skr = (Q + qps - 1) / qps;
                const long nwg = tiles * skr;
                const double rounds = ceil((double)nwg / 256.0);
                double t = rounds * (3.0 * qps * c_step + 2500.0 + ((steps1 + skr - 1) / skr) * 1.6 * c_step + (steps1 && skr > 1 ? 800.0 : 0.0));
                if (skr > 1) t += 6000.0 + (double)M * cout_pad * 4.0 * skr * 2.0 / 2500.0;
                if (steps1 && skr > 1 && !halo_skip_split_enabled()) continue;
                if (tall_mode() == 2 && cout_pad % 128 == 0) t = 1e31;           // mode 2: only where the 128-cout tile cannot run
                if (tall_mode() == 3 && skr == 1 && best.halo == 1 && best.splitk == 1) t = 0.0;   // mode 3 (experiments): wherever the 128-cout tile runs unsplit
                if (t < best_t) { best_t = t; best = ConvCfg{4, 1, 64, skr}; best.halo = 2; best.mtps = mtps; best.qps = qps; }
            }
        }
        return best;
    }
    // Whether conv3_halo_kernel (and with it the cube and plane kernels) can take the conv whose geometry, sources and skip c holds: 3^3,
    // stride 1, pad 1, same size, one main source, K steps of 64 channels; with a fused skip only where LDM_HALO_SKIP admits it, and a
    // skip under a forced K split (operator entries; 0 = the planner's) only where LDM_HALO_SKIP_SPLIT does
    static bool conv_halo_ok(const ConvRec& c, int bk, int forced_split) {
        return c.k == 3 && c.stride == 1 && c.pad == 1 && !c.ups && !c.exact && c.cb == 0 && bk == 64 &&
               c.Din == c.Dout && c.Hin == c.Hout && c.Win == c.Wout &&
               (c.c1a + c.c1b == 0 || (halo_skip_enabled() && (forced_split <= 1 || halo_skip_split_enabled())));
    }
    // Two workgroups per CU on the general kernel: with 32-channel K steps a 128-row tile runs on four waves and 78 KiB of LDS, so
    // a CU holds two and one's prologue / epilogue sits under the other's K loop.  Measured on the 96^3 phase-upsample conv of the
    // AutoencoderKL decoder (16 K steps per tile: fixed cost = half of a tile): 474 -> 328 us; 4 x 1 tiles (108 KiB) do not fit twice.
    // Short K loops only (<= 64 steps of 64 channels): the 116-step convs of the configs[3] training step lost 1 % with it.
    // The caller derives its K chunks from cc.bk afterwards.
    static void two_wg_steps(ConvCfg& cc, int steps, long mtiles, int cout_pad) {
        if (!cc.halo && !cc.plane && cc.bk == 64 && cc.wgm <= 2 && cc.splitk == 1 && two_wg_enabled() && steps <= 64 &&
            mtiles * (cout_pad / (64 * cc.wgn)) >= 512) cc.bk = 32;
    }
    // The configuration a bf16 conv launches with, for the plans (Builder::conv) and for the ldm_op_conv3d* entries.  c: geometry, sources
    // and skip; bk: the K step the channel counts allow; cube / plane: whether the caller admits those kernels; wgn / splitk: a tile shape /
    // K split the operator entry forces (0 = the planner's; wgn = 2 / 1 keep the halo kernel's 126 / 254-row tile where it applies)
    static ConvCfg pick_cfg(const ConvRec& c, int bk, bool cube, bool plane, int wgn = 0, int splitk = 0) {
        const int cin0 = c.ca + c.cb, steps0 = c.k * c.k * c.k * (cin0 / bk), steps1 = (c.c1a + c.c1b) / bk;
        const long dhwo = (long)c.Dout * c.Hout * c.Wout;
        const bool halo_ok = conv_halo_ok(c, bk, splitk);
        ConvCfg cc = choose_cfg(c.M, c.cout_pad, steps0, bk, halo_ok ? c.N : 0, dhwo, false, steps1);
        if (cube && halo_ok && cube_ok(c.Dout, c.Hout, c.Wout, cin0, c.c1a, c.c1b, c.cout_pad)) cc = cube_cfg(cin0);
        else if (plane && halo_ok && plane_ok(c.Dout, c.Hout, c.Wout, cin0, c.c1a, c.c1b, c.cout_pad)) cc = plane_cfg();
        if (wgn) {
            const bool halo = halo_ok && halo_enabled();
            cc.wgn = wgn; cc.wgm = 4 / wgn; cc.halo = (wgn == 2 && halo && c.cout_pad % 128 == 0) ? 1 : (wgn == 1 && halo && tall_mode() != 0) ? 2 : 0;
        }
        if (splitk) cc.splitk = splitk;
        if (cc.halo) {                                   // K splits of whole (kd, kh, chunk) macro steps, none empty
            const int Q = steps0 / 3;
            cc.qps = (Q + std::min(cc.splitk, Q) - 1) / std::min(cc.splitk, Q); cc.splitk = (Q + cc.qps - 1) / cc.qps;
            cc.mtps = (int)((dhwo + (cc.halo == 2 ? 253 : 125)) / (cc.halo == 2 ? 254 : 126));
        }
        if (!wgn && !splitk) two_wg_steps(cc, steps0 + steps1, conv_mtiles(c, cc), c.cout_pad);
        return cc;
    }

    // the geometry every conv-family record starts from (ConvRec); the emit site adds its operands, K chunks, tiles and flags
    static ConvRec conv_rec(const ConvArgs& a, int k, int stride, int pad, long M, int cout_real) {
        ConvRec c{}; c.N = a.xa.N; c.Din = a.xa.D; c.Hin = a.xa.H; c.Win = a.xa.W; c.Dout = a.Do; c.Hout = a.Ho; c.Wout = a.Wo;
        c.k = k; c.stride = stride; c.pad = pad; c.M = (int)M; c.couts = rup(a.w->cout, 32); c.cout_pad = a.w->cout_pad; c.cout_real = cout_real;
        return c;
    }
    // ... and the epilogue operands, where the op that gets the record applies the epilogue
    static void conv_epilogue(ConvRec& c, const ConvArgs& a, const Act& out) {
        c.bias = a.no_bias ? Ref() : w_ref(a.w->b_off); c.temb = a.temb; c.temb_stride = a.temb_stride;
        c.residual = a.residual.valid ? ws_ref(a.residual.off) : Ref();
        c.out = a.f32_out ? a.out_ref : ws_ref(out.off); c.f32_out = a.f32_out ? 1 : 0;
    }
    // ... and the sources as they are (no hi / lo split)
    static void conv_sources(ConvRec& c, const ConvArgs& a) {
        c.xa = ws_ref(a.xa.off); c.xb = a.xb.valid ? ws_ref(a.xb.off) : Ref(); c.ca = a.xa.C; c.cb = a.xb.valid ? a.xb.C : 0;
    }
    void record_conv(const ConvArgs& a, const Act& out) { if (recording) { Tape t; t.kind = 0; t.c = a; t.out = out; tape.push_back(t); } }
    // the networks' last layer (Cout <= 4, fp32 NCDHW output) on conv3_thin_kernel (conv_thin.h); x3: over the (hi | lo) split of the
    // input against [hi | lo | hi] weights (ThinParams::x3_c)
    static long thin_tiles(const ConvArgs& a) {
        return (long)a.xa.N * ((a.Do + THIN_TD - 1) / THIN_TD) * ((a.Ho + THIN_TH - 1) / THIN_TH) * ((a.Wo + THIN_TW - 1) / THIN_TW);
    }
    void emit_thin(const ConvArgs& a, long M, Ref w, int cout_real, bool x3) {
        Op op{}; op.kind = OP_CONV_THIN;
        ConvRec& c = op.cv; c = conv_rec(a, 3, 1, 1, M, cout_real); conv_epilogue(c, a, Act());
        c.xa = ws_ref(a.xa.off); c.ca = x3 ? 2 * a.xa.C : a.xa.C; c.x3 = x3; c.w = w;
        plan->ops.push_back(op);
    }
    // 1x1x1 convolution as a light GEMM (gemm_light.h; kind OP_GEMM_LIGHT32: on fp32 operands split in registers, gemm_light_x3.h):
    // tiles of 64 (big) or 32 rows, each leaving one row of the output's GroupNorm partials where they do not straddle samples
    Act emit_light(OpKind kind, const ConvArgs& a, long M, Ref w, int big, bool want_stats) {
        const int N = a.xa.N, rows = big ? 64 : 32;
        Op op{}; op.kind = kind; op.cc.big = big;
        ConvRec& c = op.cv; c = conv_rec(a, a.k, a.stride, a.pad, M, a.w->cout);
        op.cc.wg = kind == OP_GEMM_LIGHT && gemm_wg_ok(!a.xb.valid, a.xa.C + (a.xb.valid ? a.xb.C : 0), M);
        if (a.pre_gn) {
            op.cc.wg = 2; c.gamma = w_ref(a.pre_gn->g_off); c.beta = w_ref(a.pre_gn->b_off); c.gn_groups = a.pre_groups; c.gn_eps = a.pre_eps;
            c.gn_stats = ws_ref(a.xa.stats_off); c.gn_nrb = a.pre_nrb;
        }
        Act out = new_act(N, a.Do, a.Ho, a.Wo, c.couts);
        const long dhwo = (long)a.Do * a.Ho * a.Wo;
        if (want_stats && (N == 1 || dhwo % rows == 0)) {
            out.stats_off = pool.alloc((size_t)((M + rows - 1) / rows) * c.couts * 2 * 4); out.has_stats = true;
            out.stats_nrb = (int)(N == 1 ? (M + rows - 1) / rows : dhwo / rows);
        }
        conv_epilogue(c, a, out); conv_sources(c, a); c.w = w; c.stats = out.has_stats ? ws_ref(out.stats_off) : Ref();
        plan->ops.push_back(op);
        record_conv(a, out);
        return out;
    }
    // 3^3 conv with 64 (conv3_block_kernel, tiles of `th` rows) or 128 (conv3_block128_kernel, th = 8) output channels, one halo block in
    // LDS per workgroup (conv_block.h); `tiles` per sample, each leaving one row of the output's GroupNorm partials
    Act emit_conv_block(const ConvArgs& a, long M, int th, int tiles) {
        const int N = a.xa.N;
        Op op{}; op.kind = OP_CONV_BLOCK; op.cc.th = th;
        ConvRec& c = op.cv; c = conv_rec(a, 3, 1, 1, M, a.w->cout);
        Act out = new_act(N, a.Do, a.Ho, a.Wo, c.couts);
        if (a.want_stats) { out.stats_off = pool.alloc((size_t)N * tiles * c.couts * 2 * 4); out.has_stats = true; out.stats_nrb = tiles; }
        conv_epilogue(c, a, out); conv_sources(c, a);
        c.w = a.w_over.base != BASE_NULL ? a.w_over : w_ref(a.w->w_off); c.stats = out.has_stats ? ws_ref(out.stats_off) : Ref();
        plan->ops.push_back(op);
        record_conv(a, out);
        return out;
    }
    // fp32 precision: every conv form the inference plans use on conv_f32_kernel (the 1x1 skip runs as its own conv -> residual)
    // fp32 inference plans: the split-K finalize also leaves the output's GroupNorm partials (finalize_stats_f32_kernel), so the
    // GroupNorm that reads it folds them in its own launch (gn_apply's hp && fused branch) instead of a statistics pass.  LDM_FIN32_STATS=0: off.
    void fin32_stats(Op& f, Act& out, const ConvArgs& a, int N, int dhwo, int couts) {
        static const int on = ldm_xknob("LDM_FIN32_STATS", 1);
        if (!on || train || !a.want_stats || a.f32_out || couts % 4 || couts > 1024) return;
        int rows = 0;
        const int nrb = fin32_stats_blocks(N, dhwo, couts, &rows);
        out.stats_off = pool.alloc((size_t)N * nrb * couts * 2 * 4); out.has_stats = true; out.stats_nrb = nrb;
        f.cv.stats = ws_ref(out.stats_off); f.cv.stats_nrb = nrb; f.cv.stats_rows = rows;
    }
    // the fp32 finalize of a 3 x bf16 conv that left raw slabs (ConvRec::x3) over C real input channels
    void fin32_x3(const ConvArgs& a, Act& out, int C, long M, int splitk, int ntiles) {
        Op f{}; f.kind = OP_FIN32; f.cc = ConvCfg{2, 2, 32, splitk};
        ConvRec& d = f.cv; d = conv_rec(a, 3, 1, 1, M, a.f32_out && a.cout_real ? a.cout_real : a.w->cout);
        conv_epilogue(d, a, out);
        d.w = w32_ref(a.w->w_off); d.ca = C; d.nchunk0 = C / 32; d.ntiles = ntiles; d.mtiles = (int)((M + 127) / 128);
        fin32_stats(f, out, a, a.xa.N, a.Do * a.Ho * a.Wo, d.couts);
        partial_fixups.push_back(plan->ops.size()); plan->ops.push_back(f);
    }
    Act conv32(const ConvArgs& a, const std::string& tag) {
        const ConvW& w = *a.w;
        if (a.w1) { err = "fp32 precision: unsupported conv form (" + tag + ")"; return Act(); }
        const int cin0 = a.xa.C + (a.xb.valid ? a.xb.C : 0);
        if (cin0 != w.cin_s || cin0 % 16 || a.xa.C % 16) { err = "conv " + tag + ": channel bookkeeping mismatch"; return Act(); }
        const int N = a.xa.N;
        const long M = (long)N * a.Do * a.Ho * a.Wo;
        if (M >= (1L << 31)) { err = "conv " + tag + ": M too large"; return Act(); }
        // Upsample block in an inference plan, phase form (8 taps on the source grid instead of 27 on the upsampled one) as the
        // 3 x bf16 product on conv_igemm_kernel: the source is split once (hi | lo, same size), the kernel reads it as two concatenated
        // sources (hi | lo, then hi again) against phase weights [hi | hi | lo], fp32 slabs, fp32 finalize.
        {
            static const int x3_phase = ldm_xknob("LDM_X3_PHASE", 1);
            const int C = a.xa.C;
            if (x3_phase && !train && a.ups == 1 && !a.exact && a.k == 3 && a.stride == 1 && a.pad == 1 && !a.xb.valid && !a.w1 && !a.f32_out &&
                a.w_over.base == BASE_NULL && !a.xa.hl && a.Do == 2 * a.xa.D && a.Ho == 2 * a.xa.H && a.Wo == 2 * a.xa.W && phase_enabled() &&
                w.x3p_off != (size_t)-1 && x3_halo_ok(w, M, C) && a.temb.base == BASE_NULL && !a.residual.valid) {
                Act sp = new_act(N, a.xa.D, a.xa.H, a.xa.W, C); sp.hl = true;
                Op u{}; u.kind = OP_UPS_SPLIT32; u.lay.a = ws_ref(a.xa.off); u.lay.dst = ws_ref(sp.off);
                u.lay.N = N; u.lay.c_stored = C; u.lay.D = a.xa.D; u.lay.H = a.xa.H; u.lay.W = a.xa.W; u.lay.ups = 0;
                plan->ops.push_back(u);
                Op op{}; op.kind = OP_CONV;
                ConvRec& c = op.cv; c = conv_rec(a, 2, 1, 1, M, w.cout);
                c.xa = ws_ref(sp.off); c.xb = ws_ref(sp.off); c.w = Ref{BASE_W32, 2 * m->arena_bytes + w.x3p_off};
                c.ca = 2 * C; c.cb = C; c.phase = c.x3 = true;
                const int steps0 = 8 * (3 * C / 64);
                ConvCfg cc = choose_cfg(M, w.cout_pad, steps0, 64);
                if (cc.wgm > 2 || cc.splitk != 1) cc = ConvCfg{2, 2, 64, 1};
                if (w.cout_pad % (64 * cc.wgn)) cc = ConvCfg{4, 1, 64, 1};
                two_wg_steps(cc, steps0, conv_mtiles(c, cc), w.cout_pad);
                op.cc = cc; c.nchunk0 = 3 * C / cc.bk;
                Act out = new_act(N, a.Do, a.Ho, a.Wo, rup(w.cout, 32));
                partial_bytes = std::max(partial_bytes, (size_t)M * w.cout_pad * 4);
                partial_fixups.push_back(plan->ops.size()); plan->ops.push_back(op);
                fin32_x3(a, out, C, M, 1, 1);
                free_act(sp);
                return out;
            }
        }
        // Upsample block (nearest x2, then 3^3 conv) in an inference plan: one pass writes the upsampled tensor as the (hi | lo) split, the
        // conv then runs on the halo kernel like the ResBlock convs (12^3 -> 24^3, 256 channels: 258 -> ~175 us)
        if (!train && a.ups == 1 && !a.exact && a.k == 3 && a.stride == 1 && a.pad == 1 && !a.xb.valid && !a.w1 && !a.f32_out &&
            a.w_over.base == BASE_NULL && !a.xa.hl && a.Do == 2 * a.xa.D && a.Ho == 2 * a.xa.H && a.Wo == 2 * a.xa.W && x3_halo_ok(w, M, a.xa.C)) {
            Act up = new_act(N, a.Do, a.Ho, a.Wo, a.xa.C); up.hl = true;
            Op u{}; u.kind = OP_UPS_SPLIT32; u.lay.a = ws_ref(a.xa.off); u.lay.dst = ws_ref(up.off);
            u.lay.N = N; u.lay.c_stored = a.xa.C; u.lay.D = a.xa.D; u.lay.H = a.xa.H; u.lay.W = a.xa.W; u.lay.ups = 1;
            plan->ops.push_back(u);
            ConvArgs a2 = a; a2.xa = up; a2.ups = 0;
            Act out = conv32(a2, tag);
            free_act(up);
            return out;
        }
        if (a.xa.hl) {                                   // 3 x bf16 product on conv3_halo_kernel (x3_halo_ok decided it when the GroupNorm was planned)
            const int C = a.xa.C, n3 = C / 64;
            if (a.k != 3 || a.stride != 1 || a.pad != 1 || a.ups || a.exact || a.xb.valid || a.w_over.base != BASE_NULL ||
                w.x3_off == (size_t)-1 || C != w.cin_s || a.xa.D != a.Do || a.xa.H != a.Ho || a.xa.W != a.Wo || (long)M * C * 4 >= (1L << 32)) {
                err = "conv " + tag + ": hi/lo input reached a conv that cannot take it"; return Act();
            }
            ConvCfg cc = choose_cfg(M, w.cout_pad, 27 * 3 * n3, 64, N, (long)a.Do * a.Ho * a.Wo, true);
            if (!cc.halo) { err = "conv " + tag + ": no halo configuration"; return Act(); }
            const int couts = rup(w.cout, 32);
            Act out;                                         // f32_out (the network's last conv): fp32 NCDHW straight to the caller's buffer
            if (!a.f32_out) out = new_act(N, a.Do, a.Ho, a.Wo, couts);
            Op op{}; op.kind = OP_CONV; op.cc = cc;
            ConvRec& c = op.cv; c = conv_rec(a, 3, 1, 1, M, w.cout);
            c.xa = ws_ref(a.xa.off); c.w = Ref{BASE_W32, 2 * m->arena_bytes + w.x3_off};
            c.ca = 2 * C; c.x3 = true; c.nchunk0 = 3 * n3;
            static const int x3_fused = ldm_xknob("LDM_X3_FUSED_EP", 1);
            {   // the last layer with <= 4 output channels: conv3_thin_kernel over the split (conv_thin.h, ThinParams::x3_c)
                static const int thin = ldm_knob("LDM_CONV_THIN", 1);
                static const long thin_min = ldm_knob("LDM_CONV_THIN_MIN", 512L);   // the bf16 branch's threshold (Builder::conv)
                const int cr = a.cout_real ? a.cout_real : w.cout;
                if (thin && a.f32_out && cr <= 4 && C <= 128 && a.temb.base == BASE_NULL && !a.residual.valid && thin_tiles(a) >= thin_min) {
                    emit_thin(a, M, c.w, cr, true);
                    return Act();
                }
            }
            if (cc.splitk == 1 && x3_fused && a.f32_out) {   // no split, last conv: the kernel's own fp32 NCDHW epilogue (bias only)
                c.ep32_ncdhw = true; c.f32_out = 1; c.cout_real = a.cout_real ? a.cout_real : w.cout;
                c.bias = a.no_bias ? Ref() : w_ref(w.b_off); c.out = a.out_ref;
                plan->ops.push_back(op);
                return out;
            }
            if (cc.splitk == 1 && x3_fused) {                // no split: bias / time embedding / residual, the fp32 store and the GroupNorm partials in the conv's epilogue
                c.ep32_ndhwc = true; conv_epilogue(c, a, out);
                if (a.want_stats) {
                    out.stats_nrb = conv_stats_rows(c, cc);
                    out.stats_off = pool.alloc((size_t)N * out.stats_nrb * couts * 2 * 4); out.has_stats = true; c.stats = ws_ref(out.stats_off);
                }
                plan->ops.push_back(op);
                return out;
            }
            partial_bytes = std::max(partial_bytes, (size_t)cc.splitk * M * w.cout_pad * 4);
            partial_fixups.push_back(plan->ops.size()); plan->ops.push_back(op);
            fin32_x3(a, out, C, M, cc.splitk, w.cout_pad / 128 ? w.cout_pad / 128 : 1);
            return out;
        }
        // 3 x bf16 form of the product (conv_x3_kernel, K steps of 32 channels) in the INFERENCE plans wherever the channel counts allow:
        // ~5e-6 per block, 5e-5 end to end (gate 1e-3).  Training plans keep the exact fp32 MFMA: at unit weight gain the backward of
        // these networks amplifies a 1e-5 perturbation to 1e-3 of the gradient (measured), which is the whole parity budget.
        // LDM_F32_X3=0: fp32 MFMA everywhere; 2: 3 x bf16 in training plans too.
        static const int f32_x3 = ldm_knob("LDM_F32_X3", 1);
        const bool x3 = (f32_x3 == 2 || (f32_x3 == 1 && !train)) && cin0 % 32 == 0 && a.xa.C % 32 == 0;
        {   // 1x1x1 convolutions of the 3 x bf16 plans: light GEMM on the fp32 operands, no slabs and no finalize (gemm_light_x3.h).  LDM_LIGHT_X3=0: off.
            static const int light_x3 = ldm_xknob("LDM_LIGHT_X3", 1);
            static const long light_x3_max_m = ldm_xknob("LDM_LIGHT_X3_MAX_M", 4096L);   // above: conv_x3_kernel's LDS tiles (one split per tile) win: 24^3 x 512 -> 256: 61 vs 68 us
            if (light_x3 && x3 && M <= light_x3_max_m && a.k == 1 && a.stride == 1 && a.pad == 0 && !a.ups && !a.exact && !a.f32_out && !a.xa.hl && a.temb.base == BASE_NULL &&
                (!a.xb.valid || a.xb.C % 32 == 0) && w.cout_pad % 32 == 0 && a.xa.D == a.Do && a.xa.H == a.Ho && a.xa.W == a.Wo &&
                M * (long)std::max(cin0, w.cout_pad) * 4 < (1L << 31)) {
                return emit_light(OP_GEMM_LIGHT32, a, M, a.w_over.base != BASE_NULL ? a.w_over : w32_ref(w.w_off), gemm_light_x3_big(M, w.cout_pad),
                                  a.want_stats && !train);
            }
        }
        const int kb = x3 ? 32 : 16;
        const int taps = a.k * a.k * a.k, nchunk = cin0 / kb, steps = taps * nchunk;
        const int mtiles = (int)((M + 127) / 128);
        int bn = 0, sk = 0;
        conv32_cfg(M, w.cout_pad, steps, x3, &bn, &sk);
        const int ntiles = (w.cout_pad + bn - 1) / bn;
        const int couts = a.f32_out ? 0 : rup(w.cout, 32);
        Act out;
        if (!a.f32_out) out = new_act(N, a.Do, a.Ho, a.Wo, couts);
        Op op{}; op.kind = OP_CONV32; op.cc = ConvCfg{2, bn / 64, kb, sk};
        ConvRec& c = op.cv; c = conv_rec(a, a.k, a.stride, a.pad, M, a.cout_real ? a.cout_real : w.cout);
        conv_epilogue(c, a, out); conv_sources(c, a);
        c.w = a.w_over.base != BASE_NULL ? a.w_over : w32_ref(w.w_off);
        c.ups = a.ups & 1; c.exact = a.exact & 1; c.nchunk0 = nchunk; c.mtiles = mtiles; c.ntiles = ntiles;
        if (sk > 1) { partial_bytes = std::max(partial_bytes, (size_t)sk * M * w.cout_pad * 4); partial_fixups.push_back(plan->ops.size()); }
        plan->ops.push_back(op);
        if (sk > 1) { Op f = op; f.kind = OP_FIN32; fin32_stats(f, out, a, N, a.Do * a.Ho * a.Wo, couts); partial_fixups.push_back(plan->ops.size()); plan->ops.push_back(f); }
        record_conv(a, out);
        return out;
    }

    Act conv(const ConvArgs& a, std::string tag = "") {
        if (hp) return conv32(a, tag);
        const ConvW& w = *a.w;
        const int cin0 = a.xa.C + (a.xb.valid ? a.xb.C : 0);
        int bk = 64;
        if (a.xa.C % 64 || (a.xb.valid && a.xb.C % 64)) bk = 32;
        int cin1 = 0;
        if (a.w1) {
            cin1 = a.g1a.C + (a.g1b.valid ? a.g1b.C : 0);
            if (a.g1a.C % 64 || (a.g1b.valid && a.g1b.C % 64)) bk = 32;
        }
        if (cin0 != w.cin_s || (a.w1 && cin1 != a.w1->cin_s) || cin0 % 32 || cin1 % 32) {
            err = "conv " + tag + ": channel bookkeeping mismatch"; return Act();
        }
        const int N = a.xa.N;
        const long M = (long)N * a.Do * a.Ho * a.Wo;
        {   // the loaders address each source through a buffer descriptor with 32-bit byte offsets
            const long rows0 = (long)N * a.xa.D * a.xa.H * a.xa.W;
            const long big = std::max(std::max(rows0 * a.xa.C, a.xb.valid ? rows0 * a.xb.C : 0L),
                                      a.w1 ? std::max(M * a.g1a.C, a.g1b.valid ? M * a.g1b.C : 0L) : 0L) * 2;
            if (big >= (1L << 32)) { err = "conv " + tag + ": a source tensor exceeds 4 GiB (split the batch)"; return Act(); }
        }
        {   // the networks' last layer (Cout <= 4, fp32 NCDHW output): conv_thin.h; inference plans and (round 4) the training forward too
            static const int thin = ldm_knob("LDM_CONV_THIN", 1);
            static const long thin_min = ldm_knob("LDM_CONV_THIN_MIN", 512L);
            const int cr = a.cout_real ? a.cout_real : w.cout;
            if (thin && a.f32_out && a.k == 3 && a.stride == 1 && a.pad == 1 && !a.ups && !a.exact && !a.xb.valid && !a.w1 &&
                a.temb.base == BASE_NULL && !a.residual.valid && a.w_over.base == BASE_NULL && cr <= 4 && cin0 % 32 == 0 && cin0 <= 128 &&
                a.xa.D == a.Do && a.xa.H == a.Ho && a.xa.W == a.Wo &&
                // enough blocks to fill the chip and few channel chunks: measured 64 -> 1 at 96^3 247 -> ~100 us; 256 -> 4 at 24^3 (72 blocks, 8 chunks) 22 -> 44 us
                thin_tiles(a) >= thin_min) {
                emit_thin(a, M, w_ref(w.w_off), cr, false);
                record_conv(a, Act());
                return Act();
            }
        }
        // inference plans run (nearest x2 upsample -> 3^3 conv) as eight 2^3 convs on the source grid (conv_igemm.h, phase mode)
        const bool phase = a.ups == 1 && !a.exact && a.k == 3 && a.stride == 1 && a.pad == 1 && !train && !a.xb.valid && !a.w1 &&
                           a.w_over.base == BASE_NULL && w.wp_off != 0 && phase_enabled() &&
                           a.Do == 2 * a.xa.D && a.Ho == 2 * a.xa.H && a.Wo == 2 * a.xa.W;
        if (gemm_light_ok(a.k, a.stride, a.ups, cin0, !a.w1, !a.f32_out && a.temb.base == BASE_NULL) && light_enabled() &&
            a.xa.D == a.Do && a.xa.H == a.Ho && a.xa.W == a.Wo && M * (long)cin0 * 2 < (1L << 31))
            return emit_light(OP_GEMM_LIGHT, a, M, a.w_over.base != BASE_NULL ? a.w_over : w_ref(w.w_off), gemm_light_big(M, w.cout_pad), a.want_stats);
        if (a.pre_gn) { err = "conv " + tag + ": a GroupNorm prologue needs the light GEMM"; return Act(); }
        // 64 output channels over a large grid (the AutoencoderKL's full-resolution level): one halo block in LDS per workgroup (conv_block.h)
        if (conv_block_enabled() && a.k == 3 && a.stride == 1 && a.pad == 1 && a.ups == 0 && !a.exact && !a.xb.valid && !a.w1 && !a.f32_out &&
            w.cout_pad == 64 && rup(w.cout, 32) == 64 && cin0 <= conv_block_max_cin() &&      // (w_over: the data-gradient convs' flipped weights, same layout)
            a.xa.D == a.Do && a.xa.H == a.Ho && a.xa.W == a.Wo) {
            const int TH = conv_block_th();
            const int td = (a.Do + BLK_TD - 1) / BLK_TD, th = (a.Ho + TH - 1) / TH, tw = (a.Wo + BLK_TW - 1) / BLK_TW;
            static const long min_blocks = ldm_knob("LDM_CONV_BLOCK_MIN", 512L);
            if ((long)N * td * th * tw >= min_blocks) return emit_conv_block(a, M, TH, td * th * tw);
        }
        // 128 output channels (the AutoencoderKL's half-resolution level): eight-wave block kernel with double-buffered halo chunks (conv_block.h)
        if (conv_block128_enabled() && a.k == 3 && a.stride == 1 && a.pad == 1 && a.ups == 0 && !a.exact && !a.xb.valid && !a.w1 && !a.f32_out &&
            w.cout_pad == 128 && rup(w.cout, 32) == 128 && cin0 <= conv_block128_max_cin() && a.xa.D == a.Do && a.xa.H == a.Ho && a.xa.W == a.Wo) {
            const int td = (a.Do + BLK_TD - 1) / BLK_TD, th = (a.Ho + 7) / 8, tw = (a.Wo + BLK_TW - 1) / BLK_TW;
            static const long min_blocks = ldm_knob("LDM_CONV_BLOCK128_MIN", 192L);   // 128 tiles (32^3 x batch 2) leave half the CUs idle: AutoencoderKL training step 18.4 vs 18.6 ms
            // one eight-wave workgroup per CU: it pays where the tiles fit ONE round (48^3: 216 tiles: AutoencoderKL 96^3 encode 2.37 -> 2.34 ms) and
            // loses where they need several (72 x 88 x 56: 693 tiles = 2.7 rounds that take 3: configs[3] encode 6.65 -> 6.89 ms), so: <= CUs tiles
            static const long max_blocks = ldm_xknob("LDM_CONV_BLOCK128_MAX", 0L);
            const long tiles128 = (long)N * td * th * tw;
            if (tiles128 >= min_blocks && tiles128 <= (max_blocks > 0 ? max_blocks : (long)device_cus())) return emit_conv_block(a, M, 8, td * th * tw);
        }
        if (M >= (1L << 31)) { err = "conv " + tag + ": M too large"; return Act(); }
        Op op{}; op.kind = OP_CONV;
        ConvRec& c = op.cv; c = conv_rec(a, phase ? 2 : a.k, a.stride, a.pad, M, a.cout_real ? a.cout_real : w.cout);
        conv_sources(c, a);
        c.w = a.w_over.base != BASE_NULL ? a.w_over : w_ref(phase ? w.wp_off : w.w_off);
        if (a.w1) {                                                          // fused 1x1 skip
            c.x1a = ws_ref(a.g1a.off); c.c1a = a.g1a.C; c.w1 = w_ref(a.w1->w_off); c.bias2 = w_ref(a.w1->b_off);
            if (a.g1b.valid) { c.x1b = ws_ref(a.g1b.off); c.c1b = a.g1b.C; }
        }
        c.phase = phase; c.ups = !phase && (a.ups & 1); c.exact = !phase && (a.exact & 1);
        const ConvCfg cc = op.cc = pick_cfg(c, bk, !train && !phase, !train && !phase && !a.f32_out);
        c.nchunk0 = cin0 / cc.bk; c.nchunk1 = cin1 / cc.bk;
        Act out;
        if (!a.f32_out) {
            out = new_act(N, a.Do, a.Ho, a.Wo, c.couts);
            // GroupNorm partial slabs: one row per conv tile where those do not straddle samples; split-K: one per 32 output rows of the
            // whole tensor, written by the finalize (stats_nrb 0: gn_apply's blocks_of)
            const int nrb = a.want_stats ? conv_stats_rows(c, cc) : 0;
            if (a.want_stats && cc.splitk > 1) { out.stats_off = pool.alloc((size_t)((M + 31) / 32) * c.couts * 2 * 4); out.has_stats = true; }
            else if (nrb > 0) { out.stats_off = pool.alloc((size_t)N * nrb * c.couts * 2 * 4); out.has_stats = true; out.stats_nrb = nrb; }
        }
        conv_epilogue(c, a, out);
        c.stats = out.has_stats ? ws_ref(out.stats_off) : Ref();
        if (cc.splitk > 1) { partial_bytes = std::max(partial_bytes, (size_t)cc.splitk * M * w.cout_pad * 4); partial_fixups.push_back(plan->ops.size()); }
        plan->ops.push_back(op);
        if (cc.splitk > 1) { Op f = op; f.kind = OP_FINALIZE; partial_fixups.push_back(plan->ops.size()); plan->ops.push_back(f); }
        record_conv(a, out);
        return out;
    }

    // ---- split-K finalize + the GroupNorm that consumes it, in one launch (fin_gn.h) ------------------------------------------
    // Called right after conv() returned `raw`: if the plan's last op is that conv's OP_FINALIZE and one workgroup can own a whole
    // (sample, group) of the tensor, the finalize becomes an OP_FIN_GN that also writes GroupNorm(+SiLU)(raw) into *y, and the conv in
    // front of it writes its slabs planar (ConvCfg::slab_lg).  keep_raw = false: nobody else reads the un-normalised tensor (a
    // ResBlock's conv1 output): it is not written at all and its workspace block returns to the pool.
    // History: rounds 2 / 4 built this with a grid barrier / an arrival counter between the launch's workgroups and lost 10 % / 2.2 %
    // (DESIGN.md 3.2b); the group-owning form has no exchange.  LDM_FIN_GN=0 switches it off.
    static bool fin_gn_enabled() { static const int v = ldm_knob("LDM_FIN_GN", 1); return v != 0; }
    std::map<size_t, Act> prenorm;                   // un-normalised activation (by offset) -> its GroupNorm output, produced by an OP_FIN_GN
    bool fuse_fin_gn(Act& raw, bool keep_raw, const GnW& g, int groups, float eps, bool silu, Act* y) {
        if (hp || train || !fin_gn_enabled() || plan->ops.size() < 2 || !raw.valid) return false;
        Op& f = plan->ops.back();
        Op& cv = plan->ops[plan->ops.size() - 2];
        if (f.kind != OP_FINALIZE || cv.kind != OP_CONV || f.cv.f32_out || f.cv.out.base != BASE_WS || f.cv.out.off != raw.off) return false;
        const int C = raw.C, N = raw.N, DHW = raw.D * raw.H * raw.W;
        if (C != g.C || !fin_gn_ok(C, groups, DHW) || f.cv.phase) return false;      // (phase-mode convs scatter their rows: not planar)
        const int lg = fin_gn_lg(C, groups);
        // one CU streams a whole group's slabs (~40 - 50 GB/s per CU measured): it pays where that is less than what the separate finalize
        // + GroupNorm cost.  6^3 x 16 channels x 24 splits = 332 KB per group: 12.3 vs 9 + 8 us (per-op trace); 12^3 x 8 channels x 9 splits =
        // 498 KB: 21 - 25 vs 8.5 + 8 us: the 12^3 level keeps its three launches (profiles/r05_ab_fin_gn.txt)
        static const long max_kb = ldm_knob("LDM_FIN_GN_MAX_KB", 400);
        if ((long)cv.cc.splitk * DHW * (C / groups) * 4 > max_kb * 1024) return false;
        if (f.cv.cout_pad % (1 << lg)) return false;
        Act out = new_act(N, raw.D, raw.H, raw.W, C);
        f.kind = OP_FIN_GN;
        f.cv.gamma = w_ref(g.g_off); f.cv.beta = w_ref(g.b_off); f.cv.gn_out = ws_ref(out.off);
        f.cv.stats = Ref();                                                     // no statistics slab: the statistics never leave the launch
        f.cv.gn_groups = groups; f.cv.gn_silu = silu ? 1 : 0; f.cv.gn_lg = lg; f.cv.gn_eps = eps;
        f.cc.slab_lg = lg; cv.cc.slab_lg = lg; cv.cv.stats = Ref();
        if (raw.has_stats) { pool.release(raw.stats_off); raw.has_stats = false; }
        if (!keep_raw) { f.cv.out = Ref(); pool.release(raw.off); raw.valid = false; }
        *y = out;
        return true;
    }

    // ---- GroupNorm (+SiLU) over (xa | xb) -> contiguous bf16 --------------------------------------------
    // fp32 inference plans: LDM_X3_HALO (default 1) runs the 3^3 stride-1 convs behind a GroupNorm with >= LDM_X3_HALO_ROWS (default 1) output rows
    // as conv3_halo_kernel on the bf16 (hi | lo) split of the normalised tensor (ConvParams::x3_n): the GroupNorm writes the split
    // instead of fp32 values (same bytes), the conv leaves fp32 slabs, finalize_f32_kernel applies the epilogue.  Measured at 24^3:
    // 256 -> 256 channels 250 -> 160 us, 512 -> 256 493 -> 297 us (conv_x3_kernel splits every operand on its way into LDS, in every tile).
    static bool x3_halo_ok(const ConvW& w, long rows, int C) {
        static const int on = ldm_xknob("LDM_X3_HALO", 1);
        static const long min_rows = ldm_xknob("LDM_X3_HALO_ROWS", 1L);
        static const int f32_x3 = ldm_knob("LDM_F32_X3", 1);
        return on && f32_x3 != 0 && halo_enabled() && w.k == 3 && w.x3_off != (size_t)-1 && C == w.cin_s && C % 64 == 0 && rows >= min_rows &&
               rows * C * 4 < (1L << 32);                  // the halo kernel addresses its voxel operand with 32-bit byte offsets
    }
    // next3: the 3^3 stride-1 pad-1 convolution that is the ONLY reader of the result (resblock), or null
    // the input every GroupNorm-family record starts from (GnRec)
    static GnRec gn_rec(const Act& xa, const Act& xb) {
        GnRec g{}; g.xa = ws_ref(xa.off); g.xb = xb.valid ? ws_ref(xb.off) : Ref(); g.ca = xa.C; g.cb = xb.valid ? xb.C : 0;
        g.N = xa.N; g.DHW = xa.D * xa.H * xa.W;
        return g;
    }
    Act gn_apply(const GnW& g, const Act& xa, const Act& xb, int groups, float eps, bool silu, const ConvW* next3 = nullptr) {
        const int C = xa.C + (xb.valid ? xb.C : 0);
        if (C != g.C || C % 8 || (C / groups) * groups != C || xa.C % 8) { err = "groupnorm: channel mismatch"; return Act(); }
        const int DHW = xa.D * xa.H * xa.W, N = xa.N;
        size_t ab_off = 0, mr_off = 0;               // training: scale/shift and mean/rstd are saved per instance
        if (train) { ab_off = pool.alloc((size_t)N * C * 2 * 4); mr_off = pool.alloc((size_t)N * groups * 2 * 4); }
        else gnab_bytes = std::max(gnab_bytes, (size_t)N * C * 2 * 4);
        // what every op of this GroupNorm shares; inference plans keep scale/shift in the shared scratch (push_ab), where an op needs them
        GnRec rec = gn_rec(xa, xb);
        rec.gamma = w_ref(g.g_off); rec.beta = w_ref(g.b_off); rec.groups = groups; rec.eps = eps; rec.silu = silu;
        if (train) { rec.ab = ws_ref(ab_off); rec.mr = ws_ref(mr_off); }
        auto push = [&](OpKind kind, const GnRec& r) { Op o{}; o.kind = kind; o.gn = r; plan->ops.push_back(o); };
        auto push_ab = [&](OpKind kind, const GnRec& r) { if (!train) gnab_fixups.push_back(plan->ops.size()); push(kind, r); };
        auto record = [&](const Act& out) {
            if (!recording) return;
            Tape t; t.kind = 1; t.g = &g; t.xa = xa; t.xb = xb; t.out = out; t.ab_off = ab_off; t.mr_off = mr_off;
            t.groups = groups; t.silu = silu; tape.push_back(t);
        };
        auto blocks_of = [&](const Act& t) { return t.stats_nrb > 0 ? t.stats_nrb : splitk_stats_rows(N, DHW); };
        auto blocks_ok = [&](const Act& t) { return t.has_stats && blocks_of(t) > 0; };
        bool fused = blocks_ok(xa) && (!xb.valid || blocks_ok(xb));
        const int nrb_tot = fused ? blocks_of(xa) + (xb.valid ? blocks_of(xb) : 0) : 0;
        if (hp && (train || C / groups > 64 || nrb_tot > 1024)) fused = false;
        if (fused) {                                   // the producers left (sum, sum of squares) partials with the tensors
            rec.stats_a = ws_ref(xa.stats_off); rec.stats_b = xb.valid ? ws_ref(xb.stats_off) : Ref();
            rec.nrb_a = blocks_of(xa); rec.nrb_b = xb.valid ? blocks_of(xb) : 0;
        }
        // fp32 inference: fold (the producers' partials or this plan's slabs) + apply in one launch (gn32_fold_apply_kernel)
        auto fold_apply32 = [&]() {
            Act out = new_act(N, xa.D, xa.H, xa.W, C);
            out.hl = next3 && x3_halo_ok(*next3, (long)N * DHW, C);
            rec.out = ws_ref(out.off); rec.out_hl = out.hl; rec.chunks = gn_row_chunks(N, C, DHW, 256, 16, &rec.rows_per_block);
            return out;
        };
        if (hp && fused) { Act out = fold_apply32(); push(OP_GN_APPLY32, rec); return out; }
        if (fused && C / groups <= 64 && nrb_tot <= 512) {   // few slab rows: ONE launch folds them per block and applies
            Act out = new_act(N, xa.D, xa.H, xa.W, C);
            rec.out = ws_ref(out.off); rec.chunks = gn_row_chunks(N, C, DHW, gn_fused_blocks(), 32, &rec.rows_per_block);   // the slab fold is per block
            push(OP_GN_FUSED, rec);
            record(out);
            return out;
        }
        if (fused) push_ab(OP_GN_PREP, rec);           // one small reduce of the partials
        else {
            // fp32 inference plans: statistics fold + apply in one launch (gn32_fold_apply_kernel); one partial row per CU keeps the fold short
            static const bool gn32_fold = (ldm_knob("LDM_GN32_FOLD", 1) != 0);
            const bool fold32 = hp && !train && gn32_fold && C / groups <= 64;
            gn_slabs(N, C, DHW, 8, fold32 ? 256 : 512, &rec.nslab, &rec.rows_per_slab);
            gnpart_bytes = std::max(gnpart_bytes, (size_t)N * rec.nslab * C * 2 * 4);
            gnpart_fixups.push_back(plan->ops.size()); push(hp ? OP_GN_STATS32 : OP_GN_STATS, rec);
            gnpart_fixups.push_back(plan->ops.size());
            if (fold32) { Act out = fold_apply32(); push(OP_GN_APPLY32, rec); return out; }
            push_ab(OP_GN_FINALIZE, rec);
        }
        Act out = new_act(N, xa.D, xa.H, xa.W, C);
        GnRec ap = gn_rec(xa, xb); ap.silu = silu; ap.ab = rec.ab; ap.out = ws_ref(out.off);   // the apply reads the scale / shift alone
        push_ab(hp ? OP_GN_APPLY32 : OP_GN_APPLY, ap);
        record(out);
        return out;
    }

    // first conv of a network as im2col + light GEMM (inference plans; the training tape keeps the 3^3 form): r0 / r1 = the fp32
    // NCDHW inputs (x | cond).  Returns an invalid Act when the model has no derived weights for it.
    static bool im2col_enabled() { return ldm_knob("LDM_CONV_IM2COL", 1) != 0; }
    Act conv_in_im2col(const std::string& name, Ref r0, Ref r1, int N, int D, int H, int W, int cin, bool internal) {
        auto it = m->convs.find(name + ".im2col");
        if (train || hp || it == m->convs.end() || !im2col_enabled() || !light_enabled()) return Act();
        const ConvW& wi = it->second;
        Act pm = new_act(N, D, H, W, wi.cin_s);
        Op o{}; o.kind = OP_IM2COL; LayoutRec& l = o.lay; l.a = r0; l.b = r1; l.dst = ws_ref(pm.off);
        l.N = N; l.c_real = cin; l.c_stored = wi.cin_s; l.D = D; l.H = H; l.W = W; l.internal = internal;
        l.guided = guided && !internal;
        plan->ops.push_back(o);
        ConvArgs a; a.xa = pm; a.w = &wi; a.k = 1; a.pad = 0; a.Do = D; a.Ho = H; a.Wo = W;
        Act out = conv(a, name + ".im2col");
        free_act(pm);
        return out;
    }

    // ---- blocks ---------------------------------------------------------------------------------------
    Act conv3(const std::string& name, const Act& x, int stride = 1, int pad = 1, int ups = 0) {
        ConvArgs a; a.xa = x; a.w = &m->convs.at(name); a.k = 3; a.stride = stride; a.pad = pad; a.ups = ups;
        a.Do = conv_out_size(x.D, 3, stride, pad, ups); a.Ho = conv_out_size(x.H, 3, stride, pad, ups); a.Wo = conv_out_size(x.W, 3, stride, pad, ups);
        return conv(a, name);
    }

    // ResBlock (UNet: with temb; VAE: without).  xb = skip tensor concatenated after xa (up path) or invalid.
    // next_gn: the GroupNorm (no SiLU) of the attention block that reads this ResBlock's output next, or null: where conv2 is split
    // over K its finalize then also produces that GroupNorm's output (prenorm), which attention() picks up
    Act resblock(const std::string& p, const Act& xa, const Act& xb, int cout, int groups, float eps,
                 const std::string& skip_name, bool with_temb, const GnW* next_gn = nullptr) {
        const int cin = xa.C + (xb.valid ? xb.C : 0);
        // fp32 precision: the 1x1 skip projection runs as its own conv and enters conv2 as its residual (the bf16 plans fuse it
        // into conv2 as extra K steps).  A second stream for it (and for the time-embedding chain) was measured and removed: one
        // fork / join pair per step costs 5 % of the step under graph replay, fourteen cost 8 %
        Act sk;
        if (cin != cout && hp) {
            ConvArgs cs; cs.xa = xa; cs.xb = xb; cs.w = &m->convs.at(p + skip_name); cs.k = 1; cs.pad = 0;
            cs.Do = xa.D; cs.Ho = xa.H; cs.Wo = xa.W; cs.want_stats = false;
            sk = conv(cs, p + skip_name);
            if (!sk.valid) return Act();
        }
        Act h0 = gn_apply(m->gns.at(p + ".norm1"), xa, xb, groups, eps, true, &m->convs.at(p + ".conv1"));
        if (!h0.valid) return Act();
        ConvArgs c1; c1.xa = h0; c1.w = &m->convs.at(p + ".conv1"); c1.Do = xa.D; c1.Ho = xa.H; c1.Wo = xa.W;
        if (with_temb) {
            c1.temb = ws_ref(temb_all_off + (size_t)m->tproj_row.at(p) * 4); c1.temb_stride = tproj_stride;
            c1.temb_row = m->tproj_row.at(p);
        }
        Act h1 = conv(c1, p + ".conv1");
        free_act(h0);
        if (!h1.valid) return Act();
        Act h2;
        if (!fuse_fin_gn(h1, false, m->gns.at(p + ".norm2"), groups, eps, true, &h2)) {
            h2 = gn_apply(m->gns.at(p + ".norm2"), h1, Act(), groups, eps, true, &m->convs.at(p + ".conv2"));
            free_act(h1);
        }
        if (!h2.valid) return Act();
        ConvArgs c2; c2.xa = h2; c2.w = &m->convs.at(p + ".conv2"); c2.Do = xa.D; c2.Ho = xa.H; c2.Wo = xa.W;
        if (sk.valid) c2.residual = sk;
        else if (cin != cout) { c2.g1a = xa; c2.g1b = xb; c2.w1 = &m->convs.at(p + skip_name); }
        else { if (xb.valid) { err = "resblock: identity skip with concat input"; return Act(); } c2.residual = xa; }
        Act out = conv(c2, p + ".conv2");
        free_act(h2);
        if (sk.valid) free_act(sk);
        if (next_gn && out.valid && tap_mode != 2) {
            Act yn;
            if (fuse_fin_gn(out, true, *next_gn, groups, eps, false, &yn)) prenorm[out.off] = yn;
        }
        return out;
    }

    // GroupNorm -> qkv (1x1) -> attention -> out_proj (1x1) + x.  The fp32 plans differ in the op kind and its x3 flag; only the bf16 plans
    // pick up a GroupNorm output the previous finalize left (prenorm) and skip the qkv conv's GroupNorm partials
    Act attention(const std::string& p, const Act& x, int head_ch, int groups, float eps) {
        const int C = x.C;
        if (head_ch <= 0) head_ch = C;                  // single head (AutoencoderKL attention blocks)
        if (C % head_ch || (head_ch != 32 && head_ch != 64 && head_ch != 128 && head_ch != 256)) {
            err = "attention: head dimension must be 32, 64, 128 or 256 (" + p + (hp ? "" : ": " + std::to_string(head_ch)) + ")"; return Act();
        }
        Act hn;
        if (!hp) { auto it = prenorm.find(x.off); if (it != prenorm.end()) { hn = it->second; prenorm.erase(it); } }
        ConvArgs q; q.w = &m->convs.at(p + ".attn.qkv"); q.k = 1; q.pad = 0; q.Do = x.D; q.Ho = x.H; q.Wo = x.W;
        // inference plans whose producer left few partial rows (conv3_plane_kernel: one per z-plane): the GroupNorm runs in the prologue of
        // the q|k|v GEMM (gemm_wg.h) instead of a launch of its own, and the normalised tensor is never written.  Training plans keep it (the
        // tape needs the tensor and ab / mr), as do the fp32 plans, the tap plans and the shapes conv() would not hand to gemm_wg_kernel.
        bool fold = false;
        if (!hn.valid && !hp && !train && tap_mode == 0 && x.has_stats && x.stats_nrb > 0 && C == q.w->cin_s && C == m->gns.at(p + ".norm").C) {
            const long dhw = (long)x.D * x.H * x.W, M = x.N * dhw;
            fold = light_enabled() && gemm_light_ok(1, 1, 0, C, true, true) && M * (long)C * 2 < (1L << 31) && gemm_wg_ok(true, C, M) &&
                   gemm_wg_gn_ok(C, dhw, groups, x.stats_nrb, gemm_light_big(M, q.w->cout_pad));
        }
        if (fold) { hn = x; q.pre_gn = &m->gns.at(p + ".norm"); q.pre_groups = groups; q.pre_nrb = x.stats_nrb; q.pre_eps = eps; }
        if (!hn.valid) hn = gn_apply(m->gns.at(p + ".norm"), x, Act(), groups, eps, false);
        if (!hn.valid) return Act();
        q.xa = hn;
        if (!hp) q.want_stats = false;
        Act qkv = conv(q, p + ".qkv");
        if (!fold) free_act(hn);
        if (!qkv.valid) return Act();
        Act o = new_act(x.N, x.D, x.H, x.W, C);
        Op op{}; op.kind = hp ? OP_ATTN32 : OP_ATTN; AttnRec& at = op.at; at.qkv = ws_ref(qkv.off); at.out = ws_ref(o.off);
        at.B = x.N; at.N = x.D * x.H * x.W; at.C = C; at.heads = C / head_ch; at.d = head_ch; at.scale = 1.0f / sqrtf((float)head_ch);
        if (hp) {
            // inference plans: QK^T and PV as 3 x bf16 MFMAs on hi / lo splits (f32_path.h, X3), like their convolutions; LDM_ATTN_X3=0: the exact fp32 MFMA
            static const int attn_x3 = ldm_knob("LDM_ATTN_X3", 1);
            at.x3 = !train && attn_x3 && ldm_knob("LDM_F32_X3", 1) != 0;
        }
        size_t lse_off = 0;
        if (train) { lse_off = pool.alloc((size_t)x.N * at.heads * at.N * 4); at.lse = ws_ref(lse_off); }
        plan->ops.push_back(op);
        if (recording) { Tape t; t.kind = 2; t.qkv = qkv; t.o = o; t.lse_off = lse_off; t.head_ch = head_ch; tape.push_back(t); }
        free_act(qkv);
        ConvArgs pr; pr.xa = o; pr.w = &m->convs.at(p + ".attn.out_proj"); pr.k = 1; pr.pad = 0;
        pr.Do = x.D; pr.Ho = x.H; pr.Wo = x.W; pr.residual = x;
        Act out = conv(pr, p + ".out_proj");
        free_act(o);
        return out;
    }

    // ---- backward pass (training plans) -------------------------------------------------------------------
    // Gradients w.r.t. activations are bf16 NDHWC tensors in the same workspace; gslot maps a forward activation
    // (by offset) to the tensor holding the sum of the contributions emitted so far.  Kernels that can add an
    // incoming gradient while they write (conv epilogue `residual`, GroupNorm backward `acc`) always write to a
    // fresh buffer; plain pass-through contributions (identity skips) alias the producer's buffer.
    // Parameter gradients go to one flat fp32 buffer (BASE_IO4) in parameter order, MONAI tensor layouts.
    std::map<size_t, Act> gslot;
    size_t dw_off = 0, vec_off = 0, dtemb_off = 0;     // staging of the conv being differentiated (fresh per conv: exports run at the end)
    std::vector<ExportDesc> exp_descs; std::vector<int2> exp_map;
    std::vector<WtDesc> wt_descs; std::vector<int2> wt_map;
    size_t sin_off = 0, e1_off = 0, e2_off = 0;      // saved time-embedding MLP activations
    static Ref grad_ref(int64_t elem_off) { Ref r; r.base = BASE_IO4; r.off = (size_t)elem_off * 4; return r; }

    Act take_grad(const Act& a) const { auto it = gslot.find(a.off); return it == gslot.end() ? Act() : it->second; }
    void add_grad_alias(const Act& target, const Act& g) {
        Act cur = take_grad(target);
        if (!cur.valid) { gslot[target.off] = g; return; }
        Act sum = new_act(g.N, g.D, g.H, g.W, g.C);
        Op o{}; o.kind = OP_ADD; o.el.a = ws_ref(cur.off); o.el.b = ws_ref(g.off); o.el.out = ws_ref(sum.off);
        o.el.n = (int)(g.rows() * g.C / (hp ? 4 : 8)); o.el.fp32 = hp;
        plan->ops.push_back(o);
        gslot[target.off] = sum;
    }
    void emit_export(size_t src_off, int taps, int rows_total, int ld, int row_off, int col_off, int cout, int cin, int64_t flat_off,
                     int nsplit = 1) {
        ExportDesc e{}; e.src_off = (long)src_off; e.dst_off = (long)flat_off; e.slab_stride = (long)taps * rows_total * ld;
        e.taps = taps; e.rows_total = rows_total; e.ld = ld; e.row_off = row_off; e.col_off = col_off; e.cout = cout; e.cin = cin; e.nsplit = nsplit;
        const int nb = ((cin + 63) / 64) * cout;
        for (int b = 0; b < nb; ++b) exp_map.push_back(make_int2((int)exp_descs.size(), b));
        exp_descs.push_back(e);
    }
    void export_conv_weights(const ConvW& w, int ld) {           // staging [taps][w.cout][ld] -> every parameter of the slot
        for (const ParamDesc& d : m->params)
            if ((d.kind == PK_CONV_W) && d.dst_off == w.w_off)
                emit_export(dw_off, d.k * d.k * d.k, w.cout, ld, d.row_off, 0, d.cout, d.cin, d.flat_off, cur_ksplit);
    }
    void export_bias(const ConvW& w) {                           // staging vector [couts] -> bias parameter(s) of the slot
        for (const ParamDesc& d : m->params)
            if (d.kind == PK_VEC_F32 && d.dst_off >= w.b_off && d.dst_off < w.b_off + (size_t)w.cout_pad * 4)
                emit_export(vec_off, 1, 1, 0, 0, (int)((d.dst_off - w.b_off) / 4), 1, d.cout, d.flat_off);
    }
    // column sums of a bf16 gradient tensor: slab partials (shared scratch) + fold
    void emit_colsum(const Act& g, bool per_sample, Ref out, int count, int out_stride) {
        const int C = g.C, DHW = g.D * g.H * g.W, N = g.N;
        int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
        const bool batched = colsum_batched() && out.base == BASE_WS;
        auto batch = [&](size_t partial_off, int rows) {                 // the finalize joins ONE batched launch (flush_colsums) in front of the
            ColsumDesc d{}; d.partial_off = (long)partial_off; d.out_off = (long)out.off; d.N = N; d.nslab = rows; d.C = C;   // first consumer of any of these sums
            d.accumulate_over_n = per_sample ? 0 : 1; d.count = count; d.out_stride = out_stride; d.gx = (count + 15) / 16;
            const int nb = d.gx * (per_sample ? N : 1);
            for (int b = 0; b < nb; ++b) cs_map.push_back(make_int2((int)cs_descs.size(), b));
            cs_descs.push_back(d);
        };
        if (g.cs_off && batched) { batch(g.cs_off, g.cs_rows); return; }   // the GroupNorm backward that wrote g left its column sums
        Op st{}; st.kind = hp ? OP_GN_STATS32 : OP_GN_STATS; st.gn = gn_rec(g, Act()); st.gn.nslab = nslab; st.gn.rows_per_slab = rps;
        if (batched) {                                                   // the partials get their own block, kept to the end of the plan
            const size_t poff = pool.alloc((size_t)N * nslab * C * 2 * 4);
            st.gn.partial = ws_ref(poff); plan->ops.push_back(st);
            batch(poff, nslab);
            return;
        }
        gnpart_bytes = std::max(gnpart_bytes, (size_t)N * nslab * C * 2 * 4);
        gnpart_fixups.push_back(plan->ops.size()); plan->ops.push_back(st);
        Op cs{}; cs.kind = OP_COLSUM; cs.gn = st.gn; cs.gn.out = out;
        cs.gn.over_n = !per_sample; cs.gn.count = count; cs.gn.out_stride = out_stride;
        gnpart_fixups.push_back(plan->ops.size()); plan->ops.push_back(cs);
    }
    std::vector<ColsumDesc> cs_descs; std::vector<int2> cs_map;
    // experiments-build switches; in the product library ldm_op_group_norm_bwd_saved (form 0 | 1) and ldm_op_colsum_finalize (batched 0 | 1)
    // compare the two forms of each
    static bool gnb_fold_enabled() { return ldm_xknob("LDM_GNB_FOLD", 1) != 0; }
    static bool colsum_batched() { return ldm_xknob("LDM_COLSUM_BATCH", 1) != 0; }
    size_t cs_flushed = 0, exp_flushed = 0;              // blocks of cs_map / exp_map already launched by an earlier flush
    void flush_colsums() {
        if (cs_map.size() > cs_flushed) {
            Op o{}; o.kind = OP_COLSUM_BATCH; o.rg.first = (int)cs_flushed; o.rg.end = (int)cs_map.size(); plan->ops.push_back(o);
            cs_flushed = cs_map.size();
        }
    }
    void flush_exports() {
        if (exp_map.size() > exp_flushed) {
            Op o{}; o.kind = OP_EXPORT_BATCH; o.rg.first = (int)exp_flushed; o.rg.end = (int)exp_map.size(); plan->ops.push_back(o);
            exp_flushed = exp_map.size();
        }
    }
    // Gradient buckets: parameters are registered in execution order, so the backward walk finishes the flat gradient buffer from
    // its end towards its front.  Whenever bucket_elems more elements are final, their staged gradients are exported and an OP_BUCKET
    // marks the range: with a communicator attached (ldm_model_set_grad_sync) its all-reduce starts there, on the comm stream, while
    // the launch stream carries on with backward (what DistributedDataParallel's bucketed hooks do: 3d_ldm/train_diffusion.py:147-149).
    int64_t bucket_hi = 0, done_from = 0;
    int64_t tail_reserved = 0;                           // parameters below this offset are produced after the tape walk (time-embedding MLP)
    static int64_t bucket_elems() { const char* e = getenv("LDM_GRAD_BUCKET_MB"); const long mb = e ? atol(e) : 48; return (int64_t)(mb < 1 ? 1 : mb) * 262144; }
    void close_bucket(bool force) {
        if (done_from >= bucket_hi) return;
        if (!force && bucket_hi - done_from < bucket_elems()) return;
        flush_colsums(); flush_exports();
        Op o{}; o.kind = OP_BUCKET; o.rg.first = (int)done_from; o.rg.count = (int)(bucket_hi - done_from); plan->ops.push_back(o);
        bucket_hi = done_from;
    }
    void emit_wgrad(const Act& dy, const Act& x, int cout, int cin, int ld, int ci_off, int k, int stride, int pad, int ups) {
        Op o{}; o.kind = OP_WGRAD;
        WgradRec& w = o.wg; w.dy = ws_ref(dy.off); w.x = ws_ref(x.off); w.dw = ws_ref(dw_off); w.cdy = dy.C; w.cx = x.C;
        w.Cout = cout; w.Cin = cin; w.dw_ld = ld; w.dw_ci_off = ci_off;
        w.N = x.N; w.Din = x.D; w.Hin = x.H; w.Win = x.W; w.Dout = dy.D; w.Hout = dy.H; w.Wout = dy.W;
        w.ksize = k; w.stride = stride; w.pad = pad; w.ups = ups; w.M = (int)dy.rows();
        w.ksplit = cur_ksplit; w.rows_total = cur_rows_total; w.fp32 = hp;
        plan->ops.push_back(o);
    }
    int cur_ksplit = 1, cur_rows_total = 0;   // voxel split / slab rows of the gradient being staged
    // dX of one source tensor `src` (channels [ci_off, ci_off + src.C) of the conv input) given dY.
    bool emit_dgrad(const Act& dy, const Act& src, const ConvW& w, int ci_off, int k, int stride, int pad, int ups) {
        if (stride == 2 && !(k == 3 && (pad == 1 || pad == 0))) { err = "backward of a stride-2 conv needs k = 3, pad 0 | 1"; return false; }
        const int taps = k * k * k;
        const int rows = rup(src.C, 64), cols = rup(w.cout, 32);
        const size_t wt_off = pool.alloc((size_t)taps * rows * cols * (hp ? 4 : 2));
        {   // transposed once per backward by the batched kernel at the head of the backward plan
            WtDesc e{}; e.src_off = (long)w.w_off; e.dst_off = (long)wt_off; e.taps = taps; e.cout = w.cout; e.cout_pad = w.cout_pad;
            e.cin = w.cin_s; e.rows = rows; e.ci_off = ci_off; e.ci_cnt = src.C; e.col_tiles = (cols + 63) / 64; e.row_tiles = rows / 64;
            const int nb = e.col_tiles * e.row_tiles * taps;
            for (int b = 0; b < nb; ++b) wt_map.push_back(make_int2((int)wt_descs.size(), b));
            wt_descs.push_back(e);
        }
        ConvW syn; syn.has = true; syn.k = k; syn.cout = src.C; syn.cout_pad = rup(src.C, 64); syn.cin_s = dy.C;
        ConvArgs d; d.xa = dy; d.w = &syn; d.w_over = ws_ref(wt_off); d.no_bias = true; d.k = k; d.stride = 1; d.pad = k - 1 - pad;
        if (stride == 2) { d.ups = 1; d.exact = 1; }
        d.Do = src.D << ups; d.Ho = src.H << ups; d.Wo = src.W << ups;
        d.want_stats = false;
        if (!ups) d.residual = take_grad(src);
        Act g = conv(d, "dgrad");
        if (!g.valid) return false;
        if (ups) {                                      // adjoint of the fused nearest x2 upsample
            Act gc = new_act(src.N, src.D, src.H, src.W, src.C);
            Op sp{}; sp.kind = OP_SUMPOOL; sp.el.a = ws_ref(g.off); sp.el.out = ws_ref(gc.off);
            sp.el.N = src.N; sp.el.D = src.D; sp.el.H = src.H; sp.el.W = src.W; sp.el.C = src.C; sp.el.fp32 = hp;
            plan->ops.push_back(sp);
            add_grad_alias(src, gc);
        } else gslot[src.off] = g;
        return true;
    }
    // Backward variants (unet_build's bwd_mode): want_params = the flat parameter gradients are produced (column sums, weight and
    // time-embedding gradients, exports, buckets); want_input = conv_in's tape entry is no leaf, the plan ends in the thin data gradient
    // that writes the caller's (dx | dcond).  !want_params is the data-only plan.
    bool want_params = true, want_input = false;
    // LDM_DGRAD_THIN=1: conv_in's data gradient on conv3_dgrad_thin_kernel (fp32 accumulators straight into the caller's tensors).  Default 0:
    // the general data-gradient conv + an unpack, 27 against 57 us at 1 x 24^3 x 256 channels (profiles/guided_step.md).  Read per plan.
    static bool dgrad_thin_enabled() { return ldm_knob("LDM_DGRAD_THIN", 0) != 0; }
    size_t thin_wp_off = 0;                              // conv_in's weights as conv3_dgrad_thin_kernel reads them (OP_DGRAD_THIN_PACK at the head of the backward)
    // dX of the network input from dY of conv_in: the (hi | lo) split of dY first in fp32 plans
    bool emit_dgrad_thin(const Act& dy, int cin_real) {
        if (cin_real > 32) { err = "input gradients: conv_in has more than 32 input channels"; return false; }
        Act src = dy;
        if (hp) {
            src = new_act(dy.N, dy.D, dy.H, dy.W, dy.C); src.hl = true;
            Op u{}; u.kind = OP_UPS_SPLIT32; u.lay.a = ws_ref(dy.off); u.lay.dst = ws_ref(src.off);
            u.lay.N = dy.N; u.lay.c_stored = dy.C; u.lay.D = dy.D; u.lay.H = dy.H; u.lay.W = dy.W; u.lay.ups = 0;
            plan->ops.push_back(u);
        }
        Op o{}; o.kind = OP_DGRAD_THIN; ConvRec& c = o.cv;
        c.xa = ws_ref(src.off); c.w = ws_ref(thin_wp_off); c.ca = dy.C; c.x3 = hp; c.cout_real = cin_real;
        c.N = dy.N; c.Din = c.Dout = dy.D; c.Hin = c.Hout = dy.H; c.Win = c.Wout = dy.W; c.k = 3; c.stride = 1; c.pad = 1;
        plan->ops.push_back(o);
        return true;
    }
    bool backward_conv(const Tape& t, const Act& dout) {
        const ConvArgs& a = t.c; const ConvW& w = *a.w;
        int cin_real = 0;
        for (const ParamDesc& d : m->params) if (d.kind == PK_CONV_W && d.dst_off == w.w_off) cin_real = d.cin;
        if (!cin_real) { err = "backward: conv slot without parameters"; return false; }
        if (dout.C != rup(w.cout, 32)) { err = "backward: gradient channel mismatch"; return false; }
        if (want_params) {
        // bias (both biases of a conv with a fused 1x1 skip see the same column sums) and the time-embedding rows
        vec_off = pool.alloc((size_t)dout.C * 4);
        emit_colsum(dout, false, ws_ref(vec_off), dout.C, 0);
        export_bias(w);
        if (a.w1) export_bias(*a.w1);
        if (a.temb_row >= 0) emit_colsum(dout, true, ws_ref(dtemb_off + (size_t)a.temb_row * 4), w.cout, tproj_stride);
        // weights
        cur_ksplit = wgrad_ksplit(dout.rows(), a.k * a.k * a.k, w.cout, cin_real, hp, a.stride, a.ups);
        cur_rows_total = w.cout;
        dw_off = pool.alloc((size_t)cur_ksplit * a.k * a.k * a.k * w.cout * cin_real * 4);
        if (a.xb.valid) {
            emit_wgrad(dout, a.xa, w.cout, a.xa.C, cin_real, 0, a.k, a.stride, a.pad, a.ups);
            emit_wgrad(dout, a.xb, w.cout, a.xb.C, cin_real, a.xa.C, a.k, a.stride, a.pad, a.ups);
        } else emit_wgrad(dout, a.xa, w.cout, cin_real, cin_real, 0, a.k, a.stride, a.pad, a.ups);
        export_conv_weights(w, cin_real);
        if (a.w1) {
            const int c1 = a.g1a.C + (a.g1b.valid ? a.g1b.C : 0);
            cur_ksplit = wgrad_ksplit(dout.rows(), 1, a.w1->cout, c1, hp); cur_rows_total = a.w1->cout;
            dw_off = pool.alloc((size_t)cur_ksplit * a.w1->cout * c1 * 4);
            emit_wgrad(dout, a.g1a, a.w1->cout, a.g1a.C, c1, 0, 1, 1, 0, 0);
            if (a.g1b.valid) emit_wgrad(dout, a.g1b, a.w1->cout, a.g1b.C, c1, a.g1a.C, 1, 1, 0, 0);
            export_conv_weights(*a.w1, c1);
        }
        }
        // data
        if (!t.leaf_input) {
            if (!emit_dgrad(dout, a.xa, w, 0, a.k, a.stride, a.pad, a.ups)) return false;
            if (a.xb.valid && !emit_dgrad(dout, a.xb, w, a.xa.C, a.k, a.stride, a.pad, a.ups)) return false;
        } else if (want_input) {
            if (dgrad_thin_enabled()) { if (!emit_dgrad_thin(dout, cin_real)) return false; }
            else {                                       // the general data gradient (faster at the headline shape: profiles/guided_step.md), then the unpack
                if (a.xb.valid) { err = "input gradients: conv_in with two sources"; return false; }
                if (!emit_dgrad(dout, a.xa, w, 0, a.k, a.stride, a.pad, a.ups)) return false;
                const Act g = take_grad(a.xa);
                Op o{}; o.kind = OP_DGRAD_UNPACK; LayoutRec& l = o.lay; l.a = ws_ref(g.off);
                l.N = g.N; l.c_real = cin_real; l.c_stored = g.C; l.DHW = g.D * g.H * g.W; l.esz = g.esz;
                plan->ops.push_back(o);
            }
        }
        if (a.w1) {
            if (!emit_dgrad(dout, a.g1a, *a.w1, 0, 1, 1, 0, 0)) return false;
            if (a.g1b.valid && !emit_dgrad(dout, a.g1b, *a.w1, a.g1a.C, 1, 1, 0, 0)) return false;
        }
        if (a.residual.valid) add_grad_alias(a.residual, dout);
        return true;
    }
    bool backward_gn(const Tape& t) {
        Act dy = take_grad(t.out);
        if (!dy.valid) { err = "backward: GroupNorm output without a gradient"; return false; }
        const Act& xa = t.xa; const Act& xb = t.xb;
        const int C = t.g->C, DHW = xa.D * xa.H * xa.W, N = xa.N;
        int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
        gnpart_bytes = std::max(gnpart_bytes, (size_t)N * nslab * C * 2 * 4);
        const size_t gsum = pool.alloc((size_t)N * t.groups * 2 * 4), dgn = pool.alloc((size_t)N * C * 4), dbn = pool.alloc((size_t)N * C * 4);
        Act acc_a = take_grad(xa), acc_b = xb.valid ? take_grad(xb) : Act();
        Act dxa = new_act(xa.N, xa.D, xa.H, xa.W, xa.C), dxb;
        if (xb.valid) dxb = new_act(xb.N, xb.D, xb.H, xb.W, xb.C);
        int64_t go = -1, bo = -1;
        for (const ParamDesc& d : m->params) {
            if (d.kind == PK_VEC_F32 && d.dst_off == t.g->g_off) go = d.flat_off;
            if (d.kind == PK_VEC_F32 && d.dst_off == t.g->b_off) bo = d.flat_off;
        }
        if (go < 0 || bo < 0) { err = "backward: GroupNorm parameters not found"; return false; }
        Op o{}; o.kind = OP_GNB;
        GnRec& r = o.gn; r = gn_rec(xa, xb);
        r.dy = ws_ref(dy.off); r.ab = ws_ref(t.ab_off); r.mr = ws_ref(t.mr_off); r.gamma = w_ref(t.g->g_off);
        r.gsum = ws_ref(gsum); r.dgamma_n = ws_ref(dgn); r.dbeta_n = ws_ref(dbn);
        r.groups = t.groups; r.silu = t.silu; r.nslab = nslab; r.rows_per_slab = rps;
        r.dgamma_flat = (int)go; r.dbeta_flat = (int)bo; r.fp32 = hp;
        if (!want_params) r.sink = ws_ref(pool.alloc((size_t)2 * C * 4));   // the kernels produce dgamma | dbeta alongside dx: nobody reads them here
        // passes 2 + 3 in one launch (gn_bwd_fold_apply_kernel) where the forward's one-launch form applies too; its blocks also leave the
        // column sums of dx per row chunk, which are the bias / time-embedding gradients of the convs that produced xa / xb (emit_colsum)
        int rpb = 0;
        const int chunks = hp || !gnb_fold_enabled() ? 0 : gnb_fold_chunks(N, C, t.groups, DHW, nslab, &rpb);
        if (chunks > 0) {
            r.rows_per_block = rpb; r.chunks = chunks;
            if (colsum_batched()) {
                const size_t cs = pool.alloc((size_t)N * chunks * C * 2 * 4);       // kept to the end of the plan, like every batched column-sum partial
                r.cs = ws_ref(cs); r.leaves_colsums = true;
                dxa.cs_off = cs; dxa.cs_rows = chunks;
                if (xb.valid) { dxb.cs_off = cs + (size_t)N * chunks * xa.C * 2 * 4; dxb.cs_rows = chunks; }
            }
        }
        r.acc_a = acc_a.valid ? ws_ref(acc_a.off) : Ref(); r.acc_b = acc_b.valid ? ws_ref(acc_b.off) : Ref();
        r.dxa = ws_ref(dxa.off); r.dxb = xb.valid ? ws_ref(dxb.off) : Ref();
        gnpart_fixups.push_back(plan->ops.size()); plan->ops.push_back(o);
        gslot[xa.off] = dxa;
        if (xb.valid) gslot[xb.off] = dxb;
        return true;
    }
    bool backward_attn(const Tape& t) {
        Act d_o = take_grad(t.o);
        if (!d_o.valid) { err = "backward: attention output without a gradient"; return false; }
        const Act& q = t.qkv;
        const int C = t.o.C, N = q.D * q.H * q.W;
        Act dqkv = new_act(q.N, q.D, q.H, q.W, q.C);
        const size_t delta = pool.alloc((size_t)q.N * (C / t.head_ch) * N * 4);
        Op o{}; o.kind = OP_ATTN_BWD; AttnRec& at = o.at;
        at.qkv = ws_ref(q.off); at.out = ws_ref(t.o.off); at.d_o = ws_ref(d_o.off); at.lse = ws_ref(t.lse_off); at.delta = ws_ref(delta);
        at.dqkv = ws_ref(dqkv.off);
        at.B = q.N; at.N = N; at.C = C; at.heads = C / t.head_ch; at.d = t.head_ch; at.fp32 = hp; at.scale = 1.0f / sqrtf((float)t.head_ch);
        plan->ops.push_back(o);
        gslot[q.off] = dqkv;
        return true;
    }
    void emit_lin_dw(Ref dy, Ref x_pre, Ref dW, Ref db, int B, int I, int O, int dy_stride, int x_stride, int silu) {
        Op o{}; o.kind = OP_LIN_DW; LinRec& l = o.lin; l.dy = dy; l.x_pre = x_pre; l.dW = dW; l.db = db;
        l.B = B; l.I = I; l.O = O; l.dy_stride = dy_stride; l.x_stride = x_stride; l.silu = silu; l.fp32 = hp;
        plan->ops.push_back(o);
    }
    void emit_lin_dx(Ref W, Ref dy, Ref x_pre, Ref dx, int B, int I, int O, int dy_stride, int x_stride, int silu) {
        const int nz = lin_dx_nz(O);
        const size_t part = pool.alloc((size_t)nz * B * I * 4);
        Op o{}; o.kind = OP_LIN_DX; LinRec& l = o.lin; l.w = W; l.dy = dy; l.x_pre = x_pre; l.dx = dx; l.part = ws_ref(part);
        l.B = B; l.I = I; l.O = O; l.dy_stride = dy_stride; l.x_stride = x_stride; l.silu = silu; l.nz = nz; l.fp32 = hp;
        plan->ops.push_back(o);
    }
    // AutoencoderKL: gradient of the fused heads conv from dz (decoder side) and the KL-term gradients (I/O 1, 2)
    Act dout_heads, vae_zin; size_t vae_ml_off = 0, vae_z_off = 0; int vae_L = 0;
    bool emit_heads_bwd() {
        Act dz = take_grad(vae_zin);
        if (!dz.valid) { err = "backward: latent without a gradient"; return false; }
        const int cs = rup(2 * vae_L, 32);
        dout_heads = new_act(dz.N, dz.D, dz.H, dz.W, cs);
        Op o{}; o.kind = OP_VAE_HEADS_BWD; ElemRec& e = o.el;
        e.dz = ws_ref(dz.off); e.ml = ws_ref(vae_ml_off); e.z = ws_ref(vae_z_off); e.g_mu = io_ref(1); e.g_sigma = io_ref(2);
        e.dy = ws_ref(dout_heads.off);
        e.N = dz.N; e.L = vae_L; e.C = cs; e.DHW = dz.D * dz.H * dz.W; e.c_dz = dz.C; e.fp32 = hp;
        plan->ops.push_back(o);
        return true;
    }
    // Walk the tape backwards.  `dout_final` = the packed gradient of the network output (the last conv writes fp32
    // NCDHW straight to the caller, so its gradient arrives through the I/O table).
    int64_t entry_param_end(const Tape& t) const {       // one past the last flat offset of the parameters this tape entry differentiates
        int64_t end = 0;
        auto upd = [&](const ParamDesc& d) { int64_t n = 1; for (auto v : d.shape) n *= v; end = std::max(end, d.flat_off + n); };
        if (t.kind == 0) {
            const ConvW& w = *t.c.w; const ConvW* w1 = t.c.w1;
            for (const ParamDesc& d : m->params) {
                const bool mine = (d.kind == PK_CONV_W && (d.dst_off == w.w_off || (w1 && d.dst_off == w1->w_off))) ||
                                  (d.kind == PK_VEC_F32 && ((d.dst_off >= w.b_off && d.dst_off < w.b_off + (size_t)w.cout_pad * 4) ||
                                                            (w1 && d.dst_off >= w1->b_off && d.dst_off < w1->b_off + (size_t)w1->cout_pad * 4)));
                if (mine) upd(d);
            }
        } else if (t.kind == 1) {
            for (const ParamDesc& d : m->params) if (d.kind == PK_VEC_F32 && (d.dst_off == t.g->g_off || d.dst_off == t.g->b_off)) upd(d);
        }
        return end;
    }
    bool backward_all(const Act& dout_final) {
        // pending_end[k] = the highest parameter end among tape entries BEFORE k: once entry k has been differentiated, the flat
        // gradient range [pending_end[k], total) is final whatever order the entries were recorded in
        std::vector<int64_t> pending_end(tape.size() + 1, 0);
        for (size_t k = 0; k < tape.size(); ++k) pending_end[k + 1] = std::max(pending_end[k], entry_param_end(tape[k]));
        for (size_t k = tape.size(); k-- > 0;) {
            const Tape& t = tape[k];
            bool ok = true;
            if (t.kind == 0) {
                if (t.c.f32_out && t.c.f32_tag == 1 && !emit_heads_bwd()) return false;
                Act dout = t.c.f32_out ? (t.c.f32_tag == 1 ? dout_heads : dout_final) : take_grad(t.out);
                if (!dout.valid) { err = "backward: conv output without a gradient"; return false; }
                ok = backward_conv(t, dout);
            } else if (t.kind == 1) ok = backward_gn(t);
            else ok = backward_attn(t);
            if (!ok) return false;
            if (!want_params) continue;
            done_from = std::min(done_from, std::max(pending_end[k], tail_reserved));
            close_bucket(false);
        }
        return true;
    }

    size_t temb_all_off = 0; int tproj_stride = 0;

    void finish() {
        // shared scratch lives ABOVE the activation pool's high-water mark: it is used throughout the plan, so it
        // must never alias a (temporarily freed) activation block
        size_t top = rup_sz(pool.high, 256);
        partial_off = top; top += rup_sz(partial_bytes, 256);
        gnpart_off = top; top += rup_sz(gnpart_bytes, 256);
        gnab_off = top; top += rup_sz(gnab_bytes, 256);
        pool.high = top;
        for (size_t k : partial_fixups) plan->ops[k].cv.partial = ws_ref(partial_off);   // conv-family ops only
        for (size_t k : gnpart_fixups) plan->ops[k].gn.partial = ws_ref(gnpart_off);     // GroupNorm-family ops only
        for (size_t k : gnab_fixups) plan->ops[k].gn.ab = ws_ref(gnab_off);
        plan->ws_bytes = pool.high + 256;
    }
};

// ================================================================================================ UNet
static int unet_register(ldm_model* m) {
    const ldm_unet_cfg& c = m->ucfg;
    const int L = c.num_levels; const int* ch = c.channels;
    const int temb = ch[0] * 4;
    for (int i = 0; i < L; ++i) if (ch[i] % 32 || ch[i] % c.norm_num_groups)
        return fail(LDM_ERR_UNSUPPORTED, "UNet channels must be multiples of 32 and of norm_num_groups (level %d: %d)", i, ch[i]);
    // Parameter (= flat gradient buffer) order follows the order in which the BACKWARD pass finishes gradients, reversed: the time
    // embedding MLP and every ResBlock's time_emb_proj come first (their gradients are the last ones produced), then conv_in, the
    // down blocks, the middle block, the up blocks and out.  The flat gradient buffer therefore fills strictly from its end to its
    // front, and the data-parallel exchange can reduce completed tail ranges while backward is still running (ldm_model_set_grad_sync).
    std::vector<std::pair<std::string, int>> tprojs;        // (resblock prefix, cout) in execution order
    bool collect = true;                                     // first pass: only list the ResBlocks (their projections are registered up front)
    auto reg_res = [&](const std::string& p, int cin, int cout) {
        if (collect) { tprojs.push_back({p, cout}); return; }
        m->reg_gn(p + ".norm1", cin);
        m->reg_conv(p + ".conv1", cin, cin, cout, 3);
        m->reg_gn(p + ".norm2", cout);
        m->reg_conv(p + ".conv2", cout, cout, cout, 3);
        if (cin != cout) m->reg_conv(p + ".skip_connection", cin, cin, cout, 1);
    };
    auto walk = [&]() {
    if (!collect) { m->reg_conv("conv_in", c.in_channels, rup(c.in_channels, 32), ch[0], 3); m->reg_im2col("conv_in", c.in_channels); }
    int oc = ch[0];
    for (int i = 0; i < L; ++i) {
        int ic = oc; oc = ch[i];
        for (int j = 0; j < c.num_res_blocks[i]; ++j) {
            char p[96]; snprintf(p, sizeof p, "down_blocks.%d.resnets.%d", i, j);
            reg_res(p, j == 0 ? ic : oc, oc);
            if (c.attention_levels[i] && !collect) { snprintf(p, sizeof p, "down_blocks.%d.attentions.%d", i, j); m->reg_attn(p, oc); }
        }
        if (i != L - 1 && !collect) { char p[96]; snprintf(p, sizeof p, "down_blocks.%d.downsampler.op", i); m->reg_conv(p, oc, oc, oc, 3); }
    }
    reg_res("middle_block.resnet_1", ch[L - 1], ch[L - 1]);
    if (!collect) m->reg_attn("middle_block.attention", ch[L - 1]);
    reg_res("middle_block.resnet_2", ch[L - 1], ch[L - 1]);
    oc = ch[L - 1];
    for (int i = 0; i < L; ++i) {
        const int lvl = L - 1 - i;
        int prev = oc; oc = ch[lvl];
        const int ic = ch[std::max(lvl - 1, 0)];
        const int nres = c.num_res_blocks[lvl] + 1;
        for (int j = 0; j < nres; ++j) {
            const int skip_c = (j == nres - 1) ? ic : oc;
            const int rin = (j == 0) ? prev : oc;
            char p[96]; snprintf(p, sizeof p, "up_blocks.%d.resnets.%d", i, j);
            reg_res(p, rin + skip_c, oc);
            if (c.attention_levels[lvl] && !collect) { snprintf(p, sizeof p, "up_blocks.%d.attentions.%d", i, j); m->reg_attn(p, oc); }
        }
        if (i != L - 1 && !collect) { char p[96]; snprintf(p, sizeof p, "up_blocks.%d.upsampler.postconv", i); m->reg_conv(p, oc, oc, oc, 3, true); }
    }
    if (!collect) { m->reg_gn("out.0", ch[0]); m->reg_conv("out.2", ch[0], ch[0], c.out_channels, 3); }
    };
    walk();                                                  // pass 1: the ResBlock list
    m->reg_linear("time_embed.0", ch[0], temb);
    m->reg_linear("time_embed.2", temb, temb);
    // stacked time_emb_proj: one GEMV for every ResBlock ([sum cout][temb] bf16)
    int rows = 0; for (auto& t : tprojs) rows += t.second;
    m->tproj_rows = rows;
    m->tproj_w_off = m->arena_alloc((size_t)rows * temb * 2);
    m->tproj_b_off = m->arena_alloc((size_t)rows * 4);
    int r = 0;
    for (auto& t : tprojs) {
        m->tproj_row[t.first] = r;
        m->reg_linear_at(t.first + ".time_emb_proj", temb, t.second, m->tproj_w_off + (size_t)r * temb * 2, m->tproj_b_off + (size_t)r * 4);
        r += t.second;
    }
    collect = false;
    walk();                                                  // pass 2: everything else, in execution order
    return 0;
}

// temb_table: the plan of ldm_unet_denoise_step when the model holds the tabulated projections of the sampler's schedule: one row copy
// (OP_TEMB_ROW) instead of sinusoid + three GEMVs; everything else (workspace layout included) is the plain forward plan
static int unet_build(ldm_model* m, int B, int D, int H, int W, Plan* plan, bool train, bool hp = false, int tap_mode = 0, bool temb_table = false,
                      bool guided = false, int bwd_mode = 1) {
    const ldm_unet_cfg& c = m->ucfg;
    const int L = c.num_levels; const int* ch = c.channels;
    const int temb = ch[0] * 4, G = c.norm_num_groups; const float eps = c.norm_eps;
    if (train && tap_mode) return fail(LDM_ERR_UNSUPPORTED, "debug taps are inference-only");
    Builder b; b.m = m; b.plan = plan; b.train = train; b.recording = train; b.hp = hp; b.tap_mode = tap_mode; b.guided = guided;
    b.want_params = (bwd_mode & 1) != 0; b.want_input = (bwd_mode & 2) != 0;
    // ---- time embedding: sinusoid -> Linear -> SiLU -> Linear -> (SiLU -> stacked projections)
    const size_t sin_off = b.pool.alloc((size_t)B * ch[0] * 4);
    const size_t e1_off = b.pool.alloc((size_t)B * temb * 4);
    const size_t e2_off = b.pool.alloc((size_t)B * temb * 4);
    b.tproj_stride = m->tproj_rows;
    b.temb_all_off = b.pool.alloc(((size_t)B * m->tproj_rows + 256) * 4);
    const LinW& l0 = m->lins.at("time_embed.0"); const LinW& l2 = m->lins.at("time_embed.2");
    if (temb_table && !train) {
        Op o{}; o.kind = OP_TEMB_ROW; o.lin.y = ws_ref(b.temb_all_off); o.lin.O = m->tproj_rows; o.lin.B = B; plan->ops.push_back(o);
    } else {
    { Op o{}; o.kind = OP_SINUSOID; o.lin.x = io_ref(2); o.lin.y = ws_ref(sin_off); o.lin.B = B; o.lin.O = ch[0];
      plan->ops.push_back(o); }
    auto gemv = [&](size_t w_off, size_t b_off, size_t x_off, size_t y_off, int I, int O, int xs, int ys, int silu) {
        Op o{}; o.kind = hp ? OP_GEMV32 : OP_GEMV; LinRec& l = o.lin;
        l.w = hp ? w32_ref(w_off) : w_ref(w_off); l.bias = w_ref(b_off); l.x = ws_ref(x_off); l.y = ws_ref(y_off);
        l.I = I; l.O = O; l.x_stride = xs; l.y_stride = ys; l.silu = silu; l.B = B; plan->ops.push_back(o);
    };
    gemv(l0.w_off, l0.b_off, sin_off, e1_off, ch[0], temb, ch[0], temb, 0);
    gemv(l2.w_off, l2.b_off, e1_off, e2_off, temb, temb, temb, temb, 1);
    gemv(m->tproj_w_off, m->tproj_b_off, e2_off, b.temb_all_off, temb, m->tproj_rows, temb, m->tproj_rows, 1);
    }

    // ---- pack input (x | cond) -> NDHWC bf16, channels padded to 32
    const int cin_s = rup(c.in_channels, 32);
    Act h = b.conv_in_im2col("conv_in", io_ref(0), io_ref(1), B, D, H, W, c.in_channels, false);
    if (!h.valid) {
        if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        Act xin = b.new_act(B, D, H, W, cin_s);
        b.pack(io_ref(0), io_ref(1), xin, c.in_channels, false);
        h = b.conv3("conv_in", xin);
        if (train && !b.tape.empty()) b.tape.back().leaf_input = true;        // no gradient w.r.t. the network input
        b.free_act(xin);
    }
    if (!h.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    b.tap("conv_in", h, ch[0]);
    std::vector<Act> skips; skips.push_back(h);
    char p[96];
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.num_res_blocks[i]; ++j) {
            snprintf(p, sizeof p, "down_blocks.%d.resnets.%d", i, j);
            char pa[96]; snprintf(pa, sizeof pa, "down_blocks.%d.attentions.%d.norm", i, j);
            Act hn = b.resblock(p, h, Act(), ch[i], G, eps, ".skip_connection", true, c.attention_levels[i] ? &m->gns.at(pa) : nullptr);
            if (!hn.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
            b.tap(p, hn, ch[i]);
            if (c.attention_levels[i]) {
                snprintf(p, sizeof p, "down_blocks.%d.attentions.%d", i, j);
                Act ha = b.attention(p, hn, c.num_head_channels[i], G, eps);
                b.free_act(hn);
                if (!ha.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
                hn = ha;
                b.tap(p, hn, ch[i]);
            }
            skips.push_back(hn); h = hn;
        }
        if (i != L - 1) {
            if ((h.D | h.H | h.W) & 1) return fail(LDM_ERR_UNSUPPORTED, "odd spatial size %dx%dx%d at a UNet downsample", h.D, h.H, h.W);
            snprintf(p, sizeof p, "down_blocks.%d.downsampler.op", i);
            Act hd = b.conv3(p, h, 2, 1);
            if (!hd.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
            b.tap(p, hd, ch[i]);
            skips.push_back(hd); h = hd;
        }
    }
    {   // middle: Res, Attn, Res.  `h` is also the last skip and stays alive.
        Act h1 = b.resblock("middle_block.resnet_1", h, Act(), ch[L - 1], G, eps, ".skip_connection", true, &m->gns.at("middle_block.attention.norm"));
        if (!h1.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        b.tap("middle_block.resnet_1", h1, ch[L - 1]);
        Act h2 = b.attention("middle_block.attention", h1, c.num_head_channels[L - 1], G, eps);
        b.free_act(h1);
        if (!h2.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        b.tap("middle_block.attention", h2, ch[L - 1]);
        Act h3 = b.resblock("middle_block.resnet_2", h2, Act(), ch[L - 1], G, eps, ".skip_connection", true);
        b.free_act(h2);
        if (!h3.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        b.tap("middle_block.resnet_2", h3, ch[L - 1]);
        h = h3;
    }
    for (int i = 0; i < L; ++i) {
        const int lvl = L - 1 - i;
        for (int j = 0; j < c.num_res_blocks[lvl] + 1; ++j) {
            Act s = skips.back(); skips.pop_back();
            snprintf(p, sizeof p, "up_blocks.%d.resnets.%d", i, j);
            char pa[96]; snprintf(pa, sizeof pa, "up_blocks.%d.attentions.%d.norm", i, j);
            Act hn = b.resblock(p, h, s, ch[lvl], G, eps, ".skip_connection", true, c.attention_levels[lvl] ? &m->gns.at(pa) : nullptr);
            b.free_act(h); b.free_act(s);
            if (!hn.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
            b.tap(p, hn, ch[lvl]);
            if (c.attention_levels[lvl]) {
                snprintf(p, sizeof p, "up_blocks.%d.attentions.%d", i, j);
                Act ha = b.attention(p, hn, c.num_head_channels[lvl], G, eps);
                b.free_act(hn);
                if (!ha.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
                hn = ha;
                b.tap(p, hn, ch[lvl]);
            }
            h = hn;
        }
        if (i != L - 1) {
            snprintf(p, sizeof p, "up_blocks.%d.upsampler.postconv", i);
            Act hu = b.conv3(p, h, 1, 1, 1);
            b.free_act(h);
            if (!hu.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
            b.tap(p, hu, ch[lvl]);
            h = hu;
        }
    }
    Act hn = b.gn_apply(m->gns.at("out.0"), h, Act(), G, eps, true, &m->convs.at("out.2"));
    b.free_act(h);
    if (!hn.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    Builder::ConvArgs oa; oa.xa = hn; oa.w = &m->convs.at("out.2"); oa.Do = D; oa.Ho = H; oa.Wo = W;
    oa.f32_out = true; oa.out_ref = io_ref(3); oa.cout_real = c.out_channels;
    b.conv(oa, "out.2");
    if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    if (train) {
        // ================= backward: reverse walk over the tape, then the time-embedding MLP =================
        plan->train = true; plan->bwd_begin = plan->ops.size();
        b.recording = false;
        const int rows = m->tproj_rows;
        b.dtemb_off = b.pool.alloc(((size_t)B * rows + 256) * 4);
        { Op o{}; o.kind = OP_WT_BATCH; o.rg.fp32 = hp; plan->ops.push_back(o); }          // every flipped / transposed weight matrix, one launch
        if (b.want_input && Builder::dgrad_thin_enabled()) {   // ... and conv_in's, as its thin data gradient reads them
            const ConvW& wi = m->convs.at("conv_in");
            const int K = (hp ? 3 : 1) * rup(wi.cout, 32);
            b.thin_wp_off = b.pool.alloc((size_t)27 * 32 * K * 2);
            Op o{}; o.kind = OP_DGRAD_THIN_PACK; ConvRec& r = o.cv;
            r.w = hp ? w32_ref(wi.w_off) : w_ref(wi.w_off); r.out = ws_ref(b.thin_wp_off);
            r.ca = rup(wi.cout, 32); r.couts = wi.cout; r.cout_pad = wi.cout_pad; r.cb = wi.cin_s; r.cout_real = c.in_channels; r.x3 = hp;
            plan->ops.push_back(o);
        }
        const int cos_ = rup(c.out_channels, 32);
        Act dout = b.new_act(B, D, H, W, cos_);
        b.pack(io_ref(0), Ref(), dout, c.out_channels, false);   // the caller passes the gradient's channel count, like the input's
        b.bucket_hi = b.done_from = m->flat_total;
        b.tail_reserved = m->params[m->pindex.at("conv_in.conv.weight")].flat_off;     // the time-embedding parameters in front of it come last
        if (!b.backward_all(dout)) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        if (b.want_params) {
        b.flush_colsums();                              // bias gradients and the time-embedding rows the MLP backward reads next
        // stacked projections  temb_all = Wt silu(e2) + bt
        const Ref dtemb = ws_ref(b.dtemb_off);
        b.dw_off = b.pool.alloc((size_t)rows * temb * 4); b.vec_off = b.pool.alloc((size_t)rows * 4);
        b.emit_lin_dw(dtemb, ws_ref(e2_off), ws_ref(b.dw_off), ws_ref(b.vec_off), B, temb, rows, rows, temb, 1);
        for (const ParamDesc& d : m->params) {
            if (d.kind == PK_LINEAR_W && d.dst_off >= m->tproj_w_off && d.dst_off < m->tproj_w_off + (size_t)rows * temb * 2)
                b.emit_export(b.dw_off, 1, rows, temb, (int)((d.dst_off - m->tproj_w_off) / ((size_t)temb * 2)), 0, d.cout, d.cin, d.flat_off);
            if (d.kind == PK_VEC_F32 && d.dst_off >= m->tproj_b_off && d.dst_off < m->tproj_b_off + (size_t)rows * 4)
                b.emit_export(b.vec_off, 1, 1, 0, 0, (int)((d.dst_off - m->tproj_b_off) / 4), 1, d.cout, d.flat_off);
        }
        const size_t de2 = b.pool.alloc((size_t)B * temb * 4), de1 = b.pool.alloc((size_t)B * temb * 4);
        b.emit_lin_dx(hp ? w32_ref(m->tproj_w_off) : w_ref(m->tproj_w_off), dtemb, ws_ref(e2_off), ws_ref(de2), B, temb, rows, rows, temb, 1);
        auto P = [&](const char* n) { return m->params[m->pindex.at(n)].flat_off; };
        // time_embed.2: e2 = L2 silu(e1) + b2;  time_embed.0: e1 = L0 sinusoid + b0
        b.emit_lin_dw(ws_ref(de2), ws_ref(e1_off), Builder::grad_ref(P("time_embed.2.weight")), Builder::grad_ref(P("time_embed.2.bias")),
                      B, temb, temb, temb, temb, 1);
        b.emit_lin_dx(hp ? w32_ref(l2.w_off) : w_ref(l2.w_off), ws_ref(de2), ws_ref(e1_off), ws_ref(de1), B, temb, temb, temb, temb, 1);
        b.emit_lin_dw(ws_ref(de1), ws_ref(sin_off), Builder::grad_ref(P("time_embed.0.weight")), Builder::grad_ref(P("time_embed.0.bias")),
                      B, ch[0], temb, temb, ch[0], 0);
        if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        b.done_from = 0; b.close_bucket(true);          // the front of the buffer: time embedding MLP, projections, whatever is left
        { Op o{}; o.kind = OP_BUCKET_JOIN; plan->ops.push_back(o); }
        }
        if (plan->wt_tab.upload(b.wt_descs, b.wt_map) || plan->exp_tab.upload(b.exp_descs, b.exp_map) ||
            (!b.cs_descs.empty() && plan->cs_tab.upload(b.cs_descs, b.cs_map)))
            return fail(LDM_ERR_HIP, "descriptor table upload failed");
    }
    b.finish();
    return 0;
}

// ================================================================================================ VAE
struct AeBlock { int kind; int a, b; };                 // 0 conv, 1 res, 2 attn, 3 down, 4 up, 5 gn
static std::vector<AeBlock> ae_encoder_layout(const ldm_vae_cfg& c) {
    std::vector<AeBlock> v; const int L = c.num_levels; const int* ch = c.channels;
    v.push_back({0, c.in_channels, ch[0]});
    int oc = ch[0];
    for (int i = 0; i < L; ++i) {
        int ic = oc; oc = ch[i];
        for (int j = 0; j < c.num_res_blocks[i]; ++j) { v.push_back({1, ic, oc}); ic = oc; if (c.attention_levels[i]) v.push_back({2, ic, ic}); }
        if (i != L - 1) v.push_back({3, ic, ic});
    }
    if (c.with_encoder_nonlocal_attn) { v.push_back({1, ch[L - 1], ch[L - 1]}); v.push_back({2, ch[L - 1], ch[L - 1]}); v.push_back({1, ch[L - 1], ch[L - 1]}); }
    v.push_back({5, ch[L - 1], ch[L - 1]});
    v.push_back({0, ch[L - 1], c.latent_channels});
    return v;
}
static std::vector<AeBlock> ae_decoder_layout(const ldm_vae_cfg& c) {
    std::vector<AeBlock> v; const int L = c.num_levels;
    std::vector<int> rev(c.channels, c.channels + L); std::reverse(rev.begin(), rev.end());
    v.push_back({0, c.latent_channels, rev[0]});
    if (c.with_decoder_nonlocal_attn) { v.push_back({1, rev[0], rev[0]}); v.push_back({2, rev[0], rev[0]}); v.push_back({1, rev[0], rev[0]}); }
    int oc = rev[0];
    for (int i = 0; i < L; ++i) {
        int ic = oc; oc = rev[i];
        const int lvl = L - 1 - i;
        for (int j = 0; j < c.num_res_blocks[lvl]; ++j) { v.push_back({1, ic, oc}); ic = oc; if (c.attention_levels[lvl]) v.push_back({2, ic, ic}); }
        if (i != L - 1) v.push_back({4, ic, ic});
    }
    v.push_back({5, oc, oc});
    v.push_back({0, oc, c.out_channels});
    return v;
}

static int vae_register(ldm_model* m) {
    const ldm_vae_cfg& c = m->vcfg;
    for (int i = 0; i < c.num_levels; ++i) if (c.channels[i] % 32 || c.channels[i] % c.norm_num_groups)
        return fail(LDM_ERR_UNSUPPORTED, "AutoencoderKL channels must be multiples of 32 and of norm_num_groups");
    auto reg = [&](const char* prefix, const std::vector<AeBlock>& lay) -> int {
        for (size_t k = 0; k < lay.size(); ++k) {
            char p[96]; snprintf(p, sizeof p, "%s.blocks.%zu", prefix, k);
            const AeBlock& bl = lay[k];
            switch (bl.kind) {
                case 0: {   // plain Convolution: keys <p>.conv.*
                    ConvW cw = m->new_conv_slot(rup(bl.a, 32), bl.b, 3);
                    m->reg_x3(cw);
                    m->reg_conv_into(p, cw, bl.a, bl.b, 3, 0, false); m->convs[p] = cw;
                    if (k == 0 && std::string(prefix) == "encoder") m->reg_im2col(p, bl.a);       // the encoder's first conv
                    break; }
                case 1:
                    m->reg_gn(std::string(p) + ".norm1", bl.a); m->reg_conv(std::string(p) + ".conv1", bl.a, bl.a, bl.b, 3);
                    m->reg_gn(std::string(p) + ".norm2", bl.b); m->reg_conv(std::string(p) + ".conv2", bl.b, bl.b, bl.b, 3);
                    if (bl.a != bl.b) m->reg_conv(std::string(p) + ".nin_shortcut", bl.a, bl.a, bl.b, 1);
                    break;
                case 2: m->reg_attn(p, bl.a); break;      // SpatialAttentionBlock, single head (d = C)
                case 3: m->reg_conv(std::string(p) + ".conv", bl.a, bl.a, bl.a, 3); break;
                case 4: m->reg_conv(std::string(p) + ".postconv", bl.a, bl.a, bl.a, 3, true); break;
                case 5: m->reg_gn(p, bl.a); break;
            }
        }
        return 0;
    };
    // parameter order = execution order (encoder, heads, post_quant_conv, decoder): the flat gradient buffer fills back to front
    LDM_TRY(reg("encoder", ae_encoder_layout(c)));
    const int Lc = c.latent_channels, Ls = rup(Lc, 32);
    ConvW heads = m->new_conv_slot(Ls, 2 * Lc, 1);                       // mu | log_sigma fused
    m->reg_conv_into("quant_conv_mu", heads, Lc, Lc, 1, 0, false);
    m->reg_conv_into("quant_conv_log_sigma", heads, Lc, Lc, 1, Lc, false);
    m->convs["quant_heads"] = heads;
    ConvW pq = m->new_conv_slot(Ls, Lc, 1);
    m->reg_conv_into("post_quant_conv", pq, Lc, Lc, 1, 0, false);
    m->convs["post_quant_conv"] = pq;
    LDM_TRY(reg("decoder", ae_decoder_layout(c)));
    return 0;
}

static int vae_run_layout(Builder& b, const char* prefix, const std::vector<AeBlock>& lay, Act h, int G, float eps,
                          bool last_f32, int io_out, Act* out, size_t k0 = 0) {
    for (size_t k = k0; k < lay.size(); ++k) {
        char p[96]; snprintf(p, sizeof p, "%s.blocks.%zu", prefix, k);
        const AeBlock& bl = lay[k];
        Act hn;
        if (bl.kind == 0) {
            const bool last = (k == lay.size() - 1);
            if (last && last_f32) {
                Builder::ConvArgs a; a.xa = h; a.w = &b.m->convs.at(p); a.Do = h.D; a.Ho = h.H; a.Wo = h.W;
                a.f32_out = true; a.out_ref = io_ref(io_out); a.cout_real = bl.b;
                b.conv(a, p); b.free_act(h);
                if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
                *out = Act(); return 0;
            }
            hn = b.conv3(p, h);
        } else if (bl.kind == 1) {
            hn = b.resblock(p, h, Act(), bl.b, G, eps, ".nin_shortcut", false);
        } else if (bl.kind == 2) {
            hn = b.attention(p, h, 0, G, eps);              // head_ch 0 = one head over all channels
        } else if (bl.kind == 3) {
            if ((h.D | h.H | h.W) & 1) return fail(LDM_ERR_UNSUPPORTED, "odd spatial size at an AutoencoderKL downsample");
            hn = b.conv3(std::string(p) + ".conv", h, 2, 0);
        } else if (bl.kind == 4) {
            hn = b.conv3(std::string(p) + ".postconv", h, 1, 1, 1);
        } else if (bl.kind == 5) {
            const ConvW* next3 = nullptr;                    // the network's last conv reads this norm (not in tapped plans: the tap would export the split)
            if (k + 1 < lay.size() && lay[k + 1].kind == 0 && b.tap_mode == 0) {
                char pn[96]; snprintf(pn, sizeof pn, "%s.blocks.%zu", prefix, k + 1);
                next3 = &b.m->convs.at(pn);
            }
            hn = b.gn_apply(b.m->gns.at(p), h, Act(), G, eps, false, next3);
        } else return fail(LDM_ERR_UNSUPPORTED, "unsupported AutoencoderKL block");
        b.free_act(h);
        if (!hn.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        b.tap(p, hn, bl.b);
        h = hn;
    }
    *out = h;
    return 0;
}

static int vae_build_encode(ldm_model* m, int B, int D, int H, int W, Plan* plan, bool hp = false, int tap_mode = 0) {
    const ldm_vae_cfg& c = m->vcfg;
    Builder b; b.m = m; b.plan = plan; b.hp = hp; b.tap_mode = tap_mode;
    const int cs = rup(c.in_channels, 32);
    Act h;
    Act first = b.conv_in_im2col("encoder.blocks.0", io_ref(0), Ref(), B, D, H, W, c.in_channels, true);
    if (first.valid) {
        b.tap("encoder.blocks.0", first, c.channels[0]);
        LDM_TRY(vae_run_layout(b, "encoder", ae_encoder_layout(c), first, c.norm_num_groups, c.norm_eps, false, 0, &h, 1));
    } else {
        if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
        Act xin = b.new_act(B, D, H, W, cs);
        b.pack(io_ref(0), Ref(), xin, c.in_channels, false);
        LDM_TRY(vae_run_layout(b, "encoder", ae_encoder_layout(c), xin, c.norm_num_groups, c.norm_eps, false, 0, &h));
    }
    // fused 1x1 heads -> fp32 [B][2L][dhw] scratch, then clamp/exp/sample
    const int dhw = h.D * h.H * h.W;
    const size_t ml_off = b.pool.alloc((size_t)B * 2 * c.latent_channels * dhw * 4);
    Builder::ConvArgs a; a.xa = h; a.w = &m->convs.at("quant_heads"); a.k = 1; a.pad = 0; a.Do = h.D; a.Ho = h.H; a.Wo = h.W;
    a.f32_out = true; a.out_ref = ws_ref(ml_off); a.cout_real = 2 * c.latent_channels;
    b.conv(a, "quant_heads");
    if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    b.free_act(h);
    { Op o{}; o.kind = OP_VAE_HEADS; ElemRec& e = o.el; e.ml = ws_ref(ml_off); e.noise = io_ref(1); e.mu = io_ref(2); e.sigma = io_ref(3); e.z = io_ref(4);
      e.N = B; e.L = c.latent_channels; e.DHW = dhw; plan->ops.push_back(o); }
    b.finish();
    return 0;
}

static int vae_build_decode(ldm_model* m, int B, int d, int h_, int w, Plan* plan, bool hp = false, int tap_mode = 0) {
    const ldm_vae_cfg& c = m->vcfg;
    Builder b; b.m = m; b.plan = plan; b.hp = hp; b.tap_mode = tap_mode;
    const int ls = rup(c.latent_channels, 32);
    Act zin = b.new_act(B, d, h_, w, ls);
    b.pack(io_ref(0), Ref(), zin, c.latent_channels, false);
    Builder::ConvArgs a; a.xa = zin; a.w = &m->convs.at("post_quant_conv"); a.k = 1; a.pad = 0; a.Do = d; a.Ho = h_; a.Wo = w;
    Act z2 = b.conv(a, "post_quant_conv");
    b.free_act(zin);
    if (!z2.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    b.tap("post_quant_conv", z2, c.latent_channels);
    Act out;
    LDM_TRY(vae_run_layout(b, "decoder", ae_decoder_layout(c), z2, c.norm_num_groups, c.norm_eps, true, 1, &out));
    b.finish();
    return 0;
}

// AutoencoderKL.forward with the tape + backward (stage-1 trainer, 3d_ldm/train_autoencoder.py:366-451):
//   forward  I/O: 0 = x, 1 = eps, 2 = z_mu, 3 = z_sigma, 5 = reconstruction
//   backward I/O: 0 = d recon, 1 = d z_mu (or null), 2 = d z_sigma (or null), 4 = flat parameter gradients
static int vae_build_train(ldm_model* m, int B, int D, int H, int W, Plan* plan, bool hp = false) {
    const ldm_vae_cfg& c = m->vcfg;
    Builder b; b.m = m; b.plan = plan; b.train = true; b.recording = true; b.hp = hp;
    const int cs = rup(c.in_channels, 32), L = c.latent_channels, ls = rup(L, 32);
    Act xin = b.new_act(B, D, H, W, cs);
    b.pack(io_ref(0), Ref(), xin, c.in_channels, true);
    const size_t t0 = b.tape.size();
    Act h;
    LDM_TRY(vae_run_layout(b, "encoder", ae_encoder_layout(c), xin, c.norm_num_groups, c.norm_eps, false, 0, &h));
    if (b.tape.size() > t0) b.tape[t0].leaf_input = true;                 // no gradient w.r.t. the image
    const int dhw = h.D * h.H * h.W;
    const size_t ml_off = b.pool.alloc((size_t)B * 2 * L * dhw * 4), z_off = b.pool.alloc((size_t)B * L * dhw * 4);
    { Builder::ConvArgs a; a.xa = h; a.w = &m->convs.at("quant_heads"); a.k = 1; a.pad = 0; a.Do = h.D; a.Ho = h.H; a.Wo = h.W;
      a.f32_out = true; a.out_ref = ws_ref(ml_off); a.cout_real = 2 * L; a.f32_tag = 1;
      b.conv(a, "quant_heads"); }
    if (!b.err.empty()) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    { Op o{}; o.kind = OP_VAE_HEADS; ElemRec& e = o.el; e.ml = ws_ref(ml_off); e.noise = io_ref(1); e.mu = io_ref(2); e.sigma = io_ref(3); e.z = ws_ref(z_off);
      e.N = B; e.L = L; e.DHW = dhw; plan->ops.push_back(o); }
    Act zin = b.new_act(B, h.D, h.H, h.W, ls);
    b.pack(ws_ref(z_off), Ref(), zin, L, true);
    Builder::ConvArgs pq; pq.xa = zin; pq.w = &m->convs.at("post_quant_conv"); pq.k = 1; pq.pad = 0; pq.Do = h.D; pq.Ho = h.H; pq.Wo = h.W;
    Act z2 = b.conv(pq, "post_quant_conv");
    if (!z2.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    Act out;
    LDM_TRY(vae_run_layout(b, "decoder", ae_decoder_layout(c), z2, c.norm_num_groups, c.norm_eps, true, 5, &out));
    // ---- backward
    plan->train = true; plan->bwd_begin = plan->ops.size();
    b.recording = false;
    b.vae_zin = zin; b.vae_ml_off = ml_off; b.vae_z_off = z_off; b.vae_L = L;
    { Op o{}; o.kind = OP_WT_BATCH; o.rg.fp32 = hp; plan->ops.push_back(o); }
    const int cos_ = rup(c.out_channels, 32);
    Act dout = b.new_act(B, D, H, W, cos_);
    b.pack(io_ref(0), Ref(), dout, c.out_channels, true);
    b.bucket_hi = b.done_from = m->flat_total;
    if (!b.backward_all(dout)) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    b.done_from = 0; b.close_bucket(true);
    { Op o{}; o.kind = OP_BUCKET_JOIN; plan->ops.push_back(o); }
    if (plan->wt_tab.upload(b.wt_descs, b.wt_map) || plan->exp_tab.upload(b.exp_descs, b.exp_map) ||
        (!b.cs_descs.empty() && plan->cs_tab.upload(b.cs_descs, b.cs_map)))
        return fail(LDM_ERR_HIP, "descriptor table upload failed");
    b.finish();
    return 0;
}

// AutoencoderKL.decode with the tape + the DATA-ONLY backward (plan kind "dec_x": image-space measurement guidance):
// the decoder half of the training plan and its arithmetic, no parameter gradient of any kind (want_params = false: no column sums,
// weight gradients, exports or buckets), and the z pack is no leaf: post_quant_conv's data gradient is unpacked into the caller's dz.
//   forward  I/O: 0 = z, 1 = reconstruction
//   backward I/O: 0 = d recon, 1 = dz
static int vae_build_decode_grad(ldm_model* m, int B, int d, int h_, int w, Plan* plan, bool hp = false) {
    const ldm_vae_cfg& c = m->vcfg;
    Builder b; b.m = m; b.plan = plan; b.train = true; b.recording = true; b.hp = hp; b.want_params = false;
    const int L = c.latent_channels, ls = rup(L, 32), f = 1 << (c.num_levels - 1);
    Act zin = b.new_act(B, d, h_, w, ls);
    b.pack(io_ref(0), Ref(), zin, L, true);
    Builder::ConvArgs pq; pq.xa = zin; pq.w = &m->convs.at("post_quant_conv"); pq.k = 1; pq.pad = 0; pq.Do = d; pq.Ho = h_; pq.Wo = w;
    Act z2 = b.conv(pq, "post_quant_conv");
    if (!z2.valid) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    Act out;
    LDM_TRY(vae_run_layout(b, "decoder", ae_decoder_layout(c), z2, c.norm_num_groups, c.norm_eps, true, 1, &out));
    // ---- backward
    plan->train = true; plan->bwd_begin = plan->ops.size();
    b.recording = false;
    { Op o{}; o.kind = OP_WT_BATCH; o.rg.fp32 = hp; plan->ops.push_back(o); }
    Act dout = b.new_act(B, d * f, h_ * f, w * f, rup(c.out_channels, 32));
    b.pack(io_ref(0), Ref(), dout, c.out_channels, true);
    if (!b.backward_all(dout)) return fail(LDM_ERR_UNSUPPORTED, "%s", b.err.c_str());
    const Act g = b.take_grad(zin);
    if (!g.valid) return fail(LDM_ERR_UNSUPPORTED, "backward: latent without a gradient");
    { Op o{}; o.kind = OP_DGRAD_UNPACK; LayoutRec& l = o.lay; l.a = ws_ref(g.off);
      l.N = g.N; l.c_real = L; l.c_stored = g.C; l.DHW = g.D * g.H * g.W; l.esz = g.esz; plan->ops.push_back(o); }
    if (plan->wt_tab.upload(b.wt_descs, b.wt_map)) return fail(LDM_ERR_HIP, "descriptor table upload failed");
    b.finish();
    return 0;
}

// ================================================================================================ launch
struct Bases { char* p[BASE_COUNT]; int sampler_steps; float guide_fill; int in_cx, in_cc; };   // sampler_steps: rows of the table behind BASE_TTAB (OP_TEMB_ROW); guide_fill: the unconditional half's condition value (LayoutRec::guided); in_cx, in_cc: channels of the caller's (dx | dcond) behind BASE_IO1 / BASE_IO2 (OP_DGRAD_THIN)
static inline char* rp(const Bases& b, const Ref& r) { return r.base == BASE_NULL ? nullptr : (b.p[r.base] ? b.p[r.base] + r.off : nullptr); }

// LDM_XCD_ROWS (tuning knob, default 0: measured 0.4 % SLOWER over the step, with and without write-through stores: DESIGN.md section 5): unsplit convolutions and the GroupNorm launches deal contiguous ROW ranges to the XCDs
// (ConvParams::tile_order 1, GnFusedParams::xcd_rows), so that a tensor is produced and consumed by the same XCD where the order of
// the work allows it; 0 = the round-2 orders (an XCD streams one weight panel; GroupNorm blocks in launch order)
static int xcd_rows_mode() { static const int v = ldm_xknob("LDM_XCD_ROWS", 0); return v; }
static inline int conv_tile_order(const ConvParams& p) { return (xcd_rows_mode() && p.splitk == 1 && !p.phase_mode) ? 1 : 0; }

template <int WGM, int WGN, int BK>
static int launch_conv_t(const ConvParams& p_in, hipStream_t s) {
    ConvParams p = p_in; p.tile_order = conv_tile_order(p);
    // 128 KiB-class LDS ring; BK = 64 tiles run 8 waves (two per SIMD, intra-workgroup K split)
    constexpr int STAGE = (64 * WGM + 64 * WGN) * BK * 2;
    constexpr int NG = (BK == 64) ? 2 : 1;
    constexpr int NS = (STAGE * 4 <= 131072) ? 4 : 3;
    constexpr int LDS = NS * STAGE + 28 * 64 * WGM * 4;       // ring + (tap, row) -> voxel table (+1 sentinel tap)
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_kernel<WGM, WGN, BK, NS, NG>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
        attr_set = true;
    }
    const int grid = p.mtiles * p.ntiles * p.splitk;
    hipLaunchKernelGGL((conv_igemm_kernel<WGM, WGN, BK, NS, NG>), dim3(grid), dim3(256 * NG), LDS, s, p);
    return 0;
}

// ---- optional HIP-event instrumentation of one conv tile configuration (bench.py's roofline leg) ----------
struct ProfState {
    bool on = false; int wgm = 0, wgn = 0, bk = 0, halo = 0;
    std::vector<hipEvent_t> ev; size_t used = 0;          // pairs (start, stop)
    std::vector<double> flops;                            // algorithmic FLOPs of each instrumented launch
    double flops_all = 0.0; long launches_all = 0;        // every conv launch while profiling is on
};
static ProfState g_prof;

static double conv_algorithmic_flops(const ConvParams& p) {
    // 2 * M * Cout_real * (k^3 * Cin0 + Cin1); input channels as stored (only the two stem convs are padded, 4 -> 32)
    const double taps = (double)p.ksize * p.ksize * p.ksize;
    return 2.0 * (double)p.M * (double)p.CoutReal * (taps * (double)(p.c0a + p.c0b) + (double)(p.c1a + p.c1b));
}

static void launch_finalize(const FinalizeParams& f, bool wt, hipStream_t s) {
    const dim3 grid((f.M + 31) / 32, (f.CoutS + 63) / 64);
    if (wt) hipLaunchKernelGGL(splitk_finalize_kernel<true>, grid, dim3(256), 0, s, f);
    else hipLaunchKernelGGL(splitk_finalize_kernel<false>, grid, dim3(256), 0, s, f);
}
static int launch_conv_impl(const ConvParams& p, const ConvCfg& cc, hipStream_t s);
static int launch_conv(const ConvParams& p, const ConvCfg& cc, hipStream_t s) {
    if (!g_prof.on) return launch_conv_impl(p, cc, s);
    g_prof.flops_all += conv_algorithmic_flops(p); g_prof.launches_all++;
    const bool hit = cc.wgm == g_prof.wgm && cc.wgn == g_prof.wgn && cc.bk == g_prof.bk && cc.halo == g_prof.halo &&
                     g_prof.used + 2 <= g_prof.ev.size();
    if (hit) HIP_TRY(hipEventRecord(g_prof.ev[g_prof.used], s));
    LDM_TRY(launch_conv_impl(p, cc, s));
    if (hit) { HIP_TRY(hipEventRecord(g_prof.ev[g_prof.used + 1], s)); g_prof.used += 2; g_prof.flops.push_back(conv_algorithmic_flops(p)); }
    return 0;
}

static int launch_conv_halo(const ConvParams& p_in, hipStream_t s, bool tall = false) {
    ConvParams p = p_in; p.tile_order = conv_tile_order(p);
    fastdiv_make((unsigned)(p.Hout * p.Wout), &p.fd_hw_m, &p.fd_hw_s); fastdiv_make((unsigned)p.Wout, &p.fd_w_m, &p.fd_w_s);
    constexpr int LDS = 6 * 16384 + 3 * 16384 + 9 * 128 * 4;
    constexpr int LDS_TALL = 6 * 8192 + 3 * 32768 + 9 * 256 * 4;
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TALL));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 0, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 0, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TALL));
        attr_set = true;
    }
    // persistent grid (conv_halo.h): at most one workgroup per CU, each walks its tiles; LDM_HALO_PERSIST=0: one workgroup per tile
    static const int persist = ldm_xknob("LDM_HALO_PERSIST", 1);
    static int cus_tab[32] = {};
    int dev_ = 0; if (hipGetDevice(&dev_) != hipSuccess || dev_ < 0 || dev_ >= 32) dev_ = 0;
    int& cus = cus_tab[dev_];
    if (!cus) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev_) == hipSuccess) cus = pr.multiProcessorCount; if (cus < 8) cus = 256; cus -= cus % 8; }
    const int tiles = p.mtiles * p.ntiles * p.splitk;
    const int grid = (persist && tiles > cus) ? cus : tiles;
    const bool loop = grid < tiles;                  // more tiles than workgroups: the persistent instantiation walks them
    static const int mi = ldm_knob("LDM_HALO_MASK_INLINE", 1);    // W-border masks between the MFMAs (conv_halo.h, MASK_INLINE)
    if (mi) {
        static bool mi_attr_tab[32] = {}; bool& mi_attr = attr_flag(mi_attr_tab);
        if (!mi_attr) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 0, false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 0, true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TALL));
            mi_attr = true;
        }
    }
    if (tall) {
        // (the tile-loop instantiations keep the masks in front: inline they push 35 - 53 registers into scratch)
        if (loop) hipLaunchKernelGGL((conv3_halo_kernel<6, 0, true, true>), dim3(grid), dim3(512), LDS_TALL, s, p);
        else if (mi) hipLaunchKernelGGL((conv3_halo_kernel<6, 0, true, false, true>), dim3(grid), dim3(512), LDS_TALL, s, p);
        else hipLaunchKernelGGL((conv3_halo_kernel<6, 0, true>), dim3(grid), dim3(512), LDS_TALL, s, p);
        return 0;
    }
#ifdef LDM_EXPERIMENTS
    // EXPERIMENTS BUILD ONLY (LDM_HALO_RW=1): the 126 x 128 tile with register-fed weights and one barrier per macro step (conv_halo_rw.h).
    // Parity-green on every conv operator test (profiles/r05_halo_rw_ops.txt) and 22 % SLOWER than conv3_halo_kernel at 24^3 (59.1 vs 47.2 us;
    // headline 443.8 vs 484.5 steps/s, profiles/r05_ab_halo_rw.txt): 16 KiB of weight fragments per K step through the vector L1 as half
    // cache lines cost ~350 cycles per step, and ONE barrier per macro step still costs ~250 cycles per step (profiles/r05_halo_ablations.txt).
    // LDM_HALO_PP=1: alternating K steps per wave group, one barrier per six K steps, weights as whole cache lines into registers
    // (conv_halo_pp.h): parity-green, 1133 cycles per K step against 823 -- bound by the vector L1's ingest of the weights
    // (profiles/r05_halo_pp_ablations.txt).  LDM_CONV_DBG bits 4 .. 256 pick its timing ablations.
    static const int pp = ldm_xknob("LDM_HALO_PP", 0);
    if (pp && !p.x3_n && !p.out_f32 && !p.out32 && !p.raw_partial && p.steps1 == 0 && p.CoutPad % 128 == 0 && (p.out || p.splitk > 1)) {
#define PP_CASE(A) if ((p.dbg & 508) == A) { \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_pp_kernel<A>), hipFuncAttributeMaxDynamicSharedMemorySize, HPP_LDS)); \
            hipLaunchKernelGGL((conv3_halo_pp_kernel<A>), dim3(tiles), dim3(512), HPP_LDS, s, p); return 0; }
        if (p.dbg & 1024) {                                  // producer-wave timing experiment: 12 waves, waves 8 - 11 issue every copy (results are wrong)
            constexpr int LDSP = 100 * 1024 + 32 * 1024;
            if (p.dbg & 32) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_pp_kernel<1200>), hipFuncAttributeMaxDynamicSharedMemorySize, LDSP));
                hipLaunchKernelGGL((conv3_halo_pp_kernel<1200>), dim3(tiles), dim3(768), LDSP, s, p); return 0;
            }
            if (p.dbg & 2) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_pp_kernel<1170>), hipFuncAttributeMaxDynamicSharedMemorySize, LDSP));
                hipLaunchKernelGGL((conv3_halo_pp_kernel<1170>), dim3(tiles), dim3(768), LDSP, s, p); return 0;
            }
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_pp_kernel<1168>), hipFuncAttributeMaxDynamicSharedMemorySize, LDSP));
            hipLaunchKernelGGL((conv3_halo_pp_kernel<1168>), dim3(tiles), dim3(768), LDSP, s, p); return 0;
        }
        PP_CASE(144) PP_CASE(4) PP_CASE(16) PP_CASE(64) PP_CASE(20) PP_CASE(68) PP_CASE(84) PP_CASE(80) PP_CASE(128) PP_CASE(256) PP_CASE(384) PP_CASE(464) PP_CASE(400) PP_CASE(208)
#undef PP_CASE
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_pp_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, HPP_LDS));
        hipLaunchKernelGGL((conv3_halo_pp_kernel<0>), dim3(tiles), dim3(512), HPP_LDS, s, p);
        return 0;
    }
    static const int rw = ldm_xknob("LDM_HALO_RW", 0);
    if (rw && !p.x3_n && !p.out_f32 && !p.out32 && !p.raw_partial && p.CoutPad % 128 == 0 && (p.out || p.splitk > 1)) {
        static bool rw_attr_tab[32] = {}; bool& rw_attr = attr_flag(rw_attr_tab);
        if (!rw_attr) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_rw_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, HRW_LDS));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_rw_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, HRW_LDS));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_rw_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, HRW_LDS));
            rw_attr = true;
        }
        if ((p.dbg & 124) == 64) { hipLaunchKernelGGL((conv3_halo_rw_kernel<64>), dim3(tiles), dim3(512), HRW_LDS, s, p); return 0; }
        if ((p.dbg & 124) == 4) { hipLaunchKernelGGL((conv3_halo_rw_kernel<4>), dim3(tiles), dim3(512), HRW_LDS, s, p); return 0; }
        hipLaunchKernelGGL((conv3_halo_rw_kernel<0>), dim3(tiles), dim3(512), HRW_LDS, s, p);
        return 0;
    }
#endif
    if (p.dbg & (4 | 8 | 16 | 32 | 64 | 128 | 256)) {      // timing ablations (operator-level API + LDM_CONV_DBG only)
#define ABL_CASE(A) if ((p.dbg & 508) == A) { \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, A>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS)); \
            hipLaunchKernelGGL((conv3_halo_kernel<6, A>), dim3(p.mtiles * p.ntiles * p.splitk), dim3(512), LDS, s, p); return 0; }
        if ((p.dbg & 508) == 384) {                            // barrier with slack 1 (dbg & 2048: slack 2): timing only, the ring protocol is NOT adapted
            constexpr int LDSX = LDS + 64;
            if (p.dbg & 2048) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 385>), hipFuncAttributeMaxDynamicSharedMemorySize, LDSX));
                hipLaunchKernelGGL((conv3_halo_kernel<6, 385>), dim3(p.mtiles * p.ntiles * p.splitk), dim3(512), LDSX, s, p); return 0;
            }
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_halo_kernel<6, 384>), hipFuncAttributeMaxDynamicSharedMemorySize, LDSX));
            hipLaunchKernelGGL((conv3_halo_kernel<6, 384>), dim3(p.mtiles * p.ntiles * p.splitk), dim3(512), LDSX, s, p); return 0;
        }
        ABL_CASE(4) ABL_CASE(8) ABL_CASE(16) ABL_CASE(12) ABL_CASE(20) ABL_CASE(24) ABL_CASE(32) ABL_CASE(40) ABL_CASE(84) ABL_CASE(68) ABL_CASE(64) ABL_CASE(128) ABL_CASE(256)
#undef ABL_CASE
    }
    if (loop) hipLaunchKernelGGL((conv3_halo_kernel<6, 0, false, true>), dim3(grid), dim3(512), LDS, s, p);
    else if (mi) hipLaunchKernelGGL((conv3_halo_kernel<6, 0, false, false, true>), dim3(grid), dim3(512), LDS, s, p);
    else hipLaunchKernelGGL((conv3_halo_kernel<6>), dim3(grid), dim3(512), LDS, s, p);
    return 0;
}

static int launch_conv_cube(const ConvParams& p, hipStream_t s) {
    if (p.c0a % 64 || p.x0b || p.x3_n || p.splitk != p.c0a / 64 || p.splitk < 2 || p.CoutPad % 16 || p.Dout > CUBE_EDGE || p.Hout > CUBE_EDGE ||
        p.Wout > CUBE_EDGE || p.c1a % 64 || p.c1b % 64 || !p.partial)
        return fail(LDM_ERR_BAD_ARG, "conv3_cube_kernel: unsupported conv (cin %d, splitk %d, %dx%dx%d)", p.c0a, p.splitk, p.Dout, p.Hout, p.Wout);
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_cube_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CUBE_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL(conv3_cube_kernel, dim3(p.splitk, p.CoutPad / 16, p.N), dim3(256), CUBE_LDS, s, p);
    return 0;
}
static int launch_conv_plane(const ConvParams& p, hipStream_t s) {
    if (p.c0a % 64 || p.c0a < 128 || p.x0b || p.x3_n || p.splitk != 1 || p.CoutPad % 16 || p.CoutS % 32 || p.Dout > PLANE_EDGE || p.Hout > PLANE_EDGE ||
        p.Wout > PLANE_EDGE || p.Dout < 1 || p.Hout < 1 || p.Wout < 1 || p.ksize != 3 || p.stride != 1 || p.pad != 1 || p.ups || p.phase_mode ||
        p.c1a % 64 || p.c1b % 64 || p.steps1 != (p.c1a + p.c1b) / 64 || !p.out || p.out_f32 || p.out32 || p.raw_partial)
        return fail(LDM_ERR_BAD_ARG, "conv3_plane_kernel: unsupported conv (cin %d, splitk %d, %dx%dx%d)", p.c0a, p.splitk, p.Dout, p.Hout, p.Wout);
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_plane_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, PLANE_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL(conv3_plane_kernel, dim3(p.CoutPad / 16, p.Dout, p.N), dim3(512), PLANE_LDS, s, p);
    return 0;
}
static int launch_conv_impl(const ConvParams& p, const ConvCfg& cc, hipStream_t s) {
    if (cc.cube) return launch_conv_cube(p, s);
    if (cc.plane) return launch_conv_plane(p, s);
    if (cc.halo) return launch_conv_halo(p, s, cc.halo == 2);
#define CASE(M_, N_, K_) if (cc.wgm == M_ && cc.wgn == N_ && cc.bk == K_) return launch_conv_t<M_, N_, K_>(p, s);
    CASE(2, 2, 64) CASE(4, 1, 64) CASE(1, 4, 64) CASE(2, 2, 32) CASE(4, 1, 32) CASE(1, 4, 32)
#undef CASE
    return fail(LDM_ERR_BAD_ARG, "no conv kernel for tile config %dx%d bk %d", cc.wgm, cc.wgn, cc.bk);
}

static inline int grid_for(long total, int per_block = 256, int cap = 4096) {
    long g = (total + per_block - 1) / per_block; if (g > cap) g = cap; if (g < 1) g = 1; return (int)g;
}

// voxel-range split of the weight-gradient GEMM: enough workgroups for 2 waves of 256 CUs, at least 16 K steps each
// ---- fp32-mode launch helpers: the plan executor and the ldm_op_*_f32 entries launch through these, so both run the same kernels
// Tile width (64 | 128 couts) and split-K of an fp32-mode conv as the planner picks them (sk normalised: no split is empty).
static void conv32_cfg(long M, int cout_pad, int steps, bool x3, int* bn_out, int* sk_out) {
    static const int f32_bn = ldm_knob("LDM_F32_BN", 0);        // tuning knobs
    static const int f32_wgs = ldm_knob("LDM_F32_WGS", 512);   // two workgroups per CU: 66 -> 73 TFLOP/s over the step
    const int mtiles = (int)((M + 127) / 128);
    int bn = (cout_pad % 128) ? 64 : 128;            // 64-wide tiles where 128 would idle half of the MFMA rows
    if (f32_bn == 64 || (f32_bn == 1 && (long)mtiles * (cout_pad / 128) < 256)) bn = 64;
    const long tiles = (long)mtiles * ((cout_pad + bn - 1) / bn);
    int sk = 1;
    if (tiles < f32_wgs * 3 / 4) {                   // fill the CUs: K split into deterministic fp32 slabs
        sk = (int)std::min<long>(std::max<long>(1, f32_wgs / tiles), std::max(1, steps / (x3 ? 4 : 8)));
        const int sps = (steps + sk - 1) / sk; sk = (steps + sps - 1) / sps;
    }
    *bn_out = bn; *sk_out = sk;
}
// Row blocks of finalize_stats_f32_kernel: returns the blocks per sample, *rows = rows per block (couts % 4 == 0, <= 1024).
static int fin32_stats_blocks(int N, int dhwo, int couts, int* rows) {
    const int cvec = couts / 4, rows_par = std::max(1, 256 / cvec);
    int nrb = std::min((dhwo + rows_par - 1) / rows_par, std::max(1, 256 / N));
    *rows = (dhwo + nrb - 1) / nrb;
    return (dhwo + *rows - 1) / *rows;
}
// conv_f32_kernel (exact fp32 MFMA) or conv_x3_kernel (3 x bf16), bn = 64 | 128 couts per tile; p.splitk > 1 leaves the slabs in p.partial
static void launch_conv32(const Conv32Params& p, bool x3, int bn, hipStream_t s) {
    const dim3 grid(p.mtiles * p.ntiles * p.splitk);
    if (x3 && bn == 128) hipLaunchKernelGGL(conv_x3_kernel<128>, grid, dim3(256), 0, s, p);
    else if (x3) hipLaunchKernelGGL(conv_x3_kernel<64>, grid, dim3(256), 0, s, p);
    else if (bn == 128) hipLaunchKernelGGL(conv_f32_kernel<128>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(conv_f32_kernel<64>, grid, dim3(256), 0, s, p);
}
// split-K slabs -> output; with p.stats_nrb > 0 also the GroupNorm (sum, sum of squares) row blocks of the stored values
static void launch_fin32(const Conv32Params& p, hipStream_t s) {
    if (p.stats_nrb > 0) hipLaunchKernelGGL(finalize_stats_f32_kernel, dim3(p.stats_nrb, p.N), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(finalize_f32_kernel, dim3(grid_for((long)p.M * (p.CoutPad / 4), 256, 4096)), dim3(256), 0, s, p);
}
static void launch_wgrad32(const Wgrad32Params& q, hipStream_t s) {
    hipLaunchKernelGGL(wgrad_f32_kernel, dim3(q.co_tiles * q.ci_tiles * q.ksize * q.ksize * q.ksize * q.ksplit), dim3(256), 0, s, q);
}
// fp32 GroupNorm(+act) backward given the forward's (a, b) and (mean, rstd): per-slab sums, fold, apply; with N > 1 the per-sample
// dgamma / dbeta rows (f.dgamma_n / f.dbeta_n) are summed into dgamma / dbeta (N == 1: the fold writes them there directly)
static void launch_gnb32(const Gnb32Params& q, const GnBwdParams& f, float* dgamma, float* dbeta, hipStream_t s) {
    const int C = q.ca + q.cb;
    hipLaunchKernelGGL(gnb32_stats_kernel, dim3(q.nslab, q.N), dim3(256), 0, s, q);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(q.groups, q.N), dim3(256), 0, s, f);
    hipLaunchKernelGGL(gnb32_apply_kernel, dim3(grid_for((long)q.N * q.DHW * (C / 4), 256, 4096)), dim3(256), 0, s, q);
    if (q.N > 1) {
        hipLaunchKernelGGL(rowsum_n_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)f.dgamma_n, dgamma, q.N, C);
        hipLaunchKernelGGL(rowsum_n_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)f.dbeta_n, dbeta, q.N, C);
    }
}
// ---- bf16 training-plan launch helpers: the plan executor and the bf16 ldm_op_* training entries launch through these
// GroupNorm(+act) backward from the forward's saved (a, b) and (mean, rstd): per-slab sums, then either the fold-apply form (chunks > 0,
// p.rows_per_block set, p.cs optional) or finalize + apply; with N > 1 the per-sample rows p.dgamma_n / p.dbeta_n are summed into
// dgamma / dbeta (N == 1: the caller points p.dgamma_n / p.dbeta_n at them)
static void launch_gnb(const GnBwdParams& p, int chunks, float* dgamma, float* dbeta, hipStream_t s) {
    const int C = p.ca + p.cb;
    hipLaunchKernelGGL(gn_bwd_stats_kernel, dim3(p.nslab, p.N), dim3(256), 0, s, p);
    if (chunks > 0) hipLaunchKernelGGL(gn_bwd_fold_apply_kernel, dim3(chunks, (C + 63) / 64, p.N), dim3(256), 0, s, p);
    else {
        hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(p.groups, p.N), dim3(256), 0, s, p);
        hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(grid_for((long)p.N * p.DHW * (C / 8), 256, 2048)), dim3(256), 0, s, p);
    }
    if (p.N > 1) {
        hipLaunchKernelGGL(rowsum_n_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)p.dgamma_n, dgamma, p.N, C);
        hipLaunchKernelGGL(rowsum_n_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)p.dbeta_n, dbeta, p.N, C);
    }
}
static void launch_colsum(const float* partial, float* out, int N, int nslab, int C, int over_n, int count, int out_stride, hipStream_t s) {
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3((count + 15) / 16, over_n ? 1 : N), dim3(256), 0, s, partial, out, N, nslab, C, over_n,
                       count, out_stride);
}
static void launch_colsum_batched(const ColsumDesc* descs, const int2* map, int nblocks, char* base, hipStream_t s) {
    hipLaunchKernelGGL(colsum_finalize_batched_kernel, dim3(nblocks), dim3(256), 0, s, descs, map, base);
}
static void launch_export(const float* src, float* dst, int taps, int rows_total, int ld, int row_off, int col_off, int cout, int cin,
                          int nsplit, long slab_stride, hipStream_t s) {
    hipLaunchKernelGGL(grad_export_kernel, dim3((cin + 63) / 64, cout), dim3(256), 0, s, src, dst, taps, rows_total, ld, row_off, col_off,
                       cout, cin, nsplit < 1 ? 1 : nsplit, slab_stride);
}
static void launch_export_batched(const ExportDesc* descs, const int2* map, int nblocks, const char* src_base, float* flat, hipStream_t s) {
    hipLaunchKernelGGL(grad_export_batched_kernel, dim3(nblocks), dim3(256), 0, s, descs, map, src_base, flat);
}
static void launch_wt_batched(const WtDesc* descs, const int2* map, int nblocks, const char* src_base, char* dst_base, hipStream_t s) {
    hipLaunchKernelGGL(weight_flip_transpose_batched_kernel, dim3(nblocks), dim3(256), 0, s, descs, map, src_base, dst_base);
}
// dx of a Linear (+ SiLU on its input): nz row slices of W into part [nz][B][I], then the fixed-order fold
static void launch_lin_dx(const bf16_t* W, const float* dy, const float* x_pre, float* dx, float* part, int B, int I, int O, int dy_stride,
                          int x_stride, int silu, int nz, hipStream_t s) {
    hipLaunchKernelGGL(linear_bwd_dx_part_kernel, dim3((I + 255) / 256, B, nz), dim3(256), 0, s, W, dy, part, I, O, dy_stride, B);
    hipLaunchKernelGGL(linear_bwd_dx_fold_kernel, dim3((I + 255) / 256, B), dim3(256), 0, s, (const float*)part, x_pre, dx, I, nz, x_stride, B, silu);
}
static void launch_lin_dw(const float* dy, const float* x_pre, float* dW, float* db, int B, int I, int O, int dy_stride, int x_stride, int silu,
                          hipStream_t s) {
    hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(grid_for((long)O * I, 256, 1 << 24)), dim3(256), 0, s, dy, x_pre, dW, db, B, I, O, dy_stride,
                       x_stride, silu);
}
static void launch_sumpool2(const bf16_t* dy, bf16_t* dx, int N, int D, int H, int W, int C, hipStream_t s) {
    hipLaunchKernelGGL(sumpool2_kernel, dim3(grid_for((long)N * D * H * W * (C / 8), 256, 2048)), dim3(256), 0, s, dy, dx, N, D, H, W, C);
}
static void launch_add_bf16(const bf16_t* a, const bf16_t* b, bf16_t* out, long nvec, hipStream_t s) {
    hipLaunchKernelGGL(add_bf16_kernel, dim3(grid_for(nvec, 256, 2048)), dim3(256), 0, s, a, b, out, nvec);
}
// ---- plan-only launch helpers: the kernels no network-level entry reaches on their own.  The plan executor, ensure_derived,
// ensure_temb_table and the ldm_op_* entries at the end of this file all launch through these, so they run the same grids.
// (x | cond) fp32 NCDHW -> zero-padded NDHWC, bf16 or fp32
static void launch_pack2(const float* x, int cx, const float* cond, int cc, void* out, int N, int Cs, int DHW, bool f32, hipStream_t s) {
    const long total = (long)N * DHW * Cs;
    if (f32) hipLaunchKernelGGL(pack2_ncdhw_f32_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, cx, cond, cc, (float*)out, N, Cs, DHW);
    else hipLaunchKernelGGL(pack2_ncdhw_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, cx, cond, cc, (bf16_t*)out, N, Cs, DHW);
}
static void launch_pack_im2col(const float* x, int cx, const float* cond, int cc, bf16_t* out, int N, int D, int H, int W, int Kp, hipStream_t s) {
    hipLaunchKernelGGL(pack_im2col_kernel, dim3(grid_for((long)N * D * H * W * (Kp / 8), 256, 16384)), dim3(256), 0, s, x, cx, cond, cc, out, N, D, H, W, Kp);
}
// conv3_thin_kernel: q carries everything but the block counts
static hipError_t launch_conv_thin(ThinParams q, hipStream_t s) {
    q.td = (q.D + THIN_TD - 1) / THIN_TD; q.th = (q.H + THIN_TH - 1) / THIN_TH; q.tw = (q.W + THIN_TW - 1) / THIN_TW;
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_thin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, THIN_LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(conv3_thin_kernel, dim3((unsigned)((long)q.N * q.td * q.th * q.tw)), dim3(256), THIN_LDS, s, q);
    return hipSuccess;
}
// conv3_dgrad_thin_kernel and the re-pack of its weights (conv_dgrad_thin.h): defined with their op entry at the end of this file, where the
// kernels are instantiated (the code object keeps the layout of every kernel that was there before them)
static void dgrad_thin_launch(const bf16_t* dy, const bf16_t* w, float* dx, float* dcond, int cx, int cc, int N, int D, int H, int W, int K, int x3_c,
                              hipStream_t s);
static void launch_dgrad_thin_pack(const void* w, bool src_f32, bf16_t* wp, int cout, int cin_real, int K, bool x3, long s_co, long s_ci, long s_tap,
                                   hipStream_t s);
// fp32 NDHWC [N][D][H][W][C] -> the (hi | lo) bf16 split, nearest x2 upsampled when up
static void launch_split_f32(const float* x, bf16_t* out, int N, int C, int D, int H, int W, int up, hipStream_t s) {
    hipLaunchKernelGGL(upsample_split_f32_kernel, dim3(grid_for(((long)N * D * H * W << (3 * up)) * (C / 4), 256, 4096)), dim3(256), 0, s, x, out, N, C, D, H, W, up);
}
// y[b][o] = W[o][:] . act(x[b][:]) + bias[o], W bf16 or fp32
static void launch_gemv(const void* w, bool f32, const float* bias, const float* x, float* y, int B, int I, int O, int x_stride, int y_stride, int silu,
                        hipStream_t s) {
    if (f32) hipLaunchKernelGGL(gemv_f32_kernel, dim3((O + 3) / 4, B), dim3(256), 0, s, (const float*)w, bias, x, y, I, O, x_stride, y_stride, silu);
    else hipLaunchKernelGGL(gemv_bf16_kernel, dim3((O + 3) / 4, B), dim3(256), 0, s, (const bf16_t*)w, bias, x, y, I, O, x_stride, y_stride, silu);
}
static void launch_sinusoid(const float* t, float* out, int B, int dim, hipStream_t s) {
    hipLaunchKernelGGL(temb_sinusoid_kernel, dim3(grid_for((long)B * dim)), dim3(256), 0, s, t, out, B, dim);
}
// weights derived from the packed [27][cout_pad][cin_s] matrices after an upload
static void launch_im2col_weights(const bf16_t* w3, bf16_t* w2, int cout_pad, int cin_s, int cin, int Kp, hipStream_t s) {
    hipLaunchKernelGGL(im2col_weights_kernel, dim3((unsigned)((cout_pad * Kp + 255) / 256)), dim3(256), 0, s, w3, w2, cout_pad, cin_s, cin, Kp);
}
static void launch_phase_weights(const bf16_t* w3, bf16_t* wp, int cout_pad, int cin_s, hipStream_t s) {
    const long vecs = (long)cout_pad * cin_s / 8;
    hipLaunchKernelGGL(phase_weights_kernel, dim3((unsigned)((vecs + 255) / 256), 64), dim3(256), 0, s, w3, wp, cout_pad, cin_s);
}
static void launch_x3_phase_weights(const float* w3, bf16_t* wp, int cout_pad, int cin, hipStream_t s) {
    hipLaunchKernelGGL(x3_phase_weights_kernel, dim3((unsigned)(((long)cout_pad * cin / 4 + 255) / 256), 64), dim3(256), 0, s, w3, wp, cout_pad, cin);
}
static void launch_x3_weights(const float* w, bf16_t* out, long rows, int cin, hipStream_t s) {
    hipLaunchKernelGGL(x3_weights_kernel, dim3(grid_for(rows * (cin / 4), 256, 2048)), dim3(256), 0, s, w, out, rows, cin);
}
static void launch_vae_heads(const float* ml, const float* eps, float* mu, float* sigma, float* z, int N, int L, int DHW, hipStream_t s) {
    hipLaunchKernelGGL(vae_heads_kernel, dim3(grid_for((long)N * L * DHW)), dim3(256), 0, s, ml, eps, mu, sigma, z, N, L, DHW);
}
template <typename T>
static void launch_vae_heads_bwd(const T* dz, int Ls, const float* ml, const float* z, const float* g_mu, const float* g_sigma, T* dy,
                                 int N, int L, int Cs, int DHW, hipStream_t s) {
    hipLaunchKernelGGL(vae_heads_bwd_kernel<T>, dim3(grid_for((long)N * DHW * Cs)), dim3(256), 0, s, dz, Ls, ml, z, g_mu, g_sigma, dy, N, L, Cs, DHW);
}
static int wgrad_pair(int taps, int cout, int cin, int stride, int ups, bool hp) {   // conv_wgrad_kernel's forms with several taps per workgroup (WgradParams::pair): 0 | 1 | 2 (three taps)
    static const int on = ldm_xknob("LDM_WGRAD_PAIR", 3);
    if (!on || hp || taps != 27) return 0;
    const bool y = on >= 2 && cout <= 64 && stride == 1 && ups == 0;
    if (cin > 64) return (y && on >= 3) ? 3 : 0;
    return y ? 2 : 1;
}
// conv_wgrad_kw3_kernel (three kw taps of a (kd, kh) per workgroup, 128 couts x 64 cins, one shared X tile): 3^3, stride 1, both channel
// counts above 64 (below, the pair forms of conv_wgrad_kernel fill the tile better).  launch_wgrad also asks for pad 1 and W >= 8.
// EXPERIMENTS BUILDS ONLY (LDM_WGRAD_KW3=1): parity-green on 11 operator cases and no faster (81.4 vs 83.8 us at 256 -> 256, 24^3): 24 % fewer
// copied bytes per MFMA bought nothing because the step is a serial sum -- copies 500 + fragment reads 500 + masks 340 + barrier 250 +
// MFMAs 900 cycles (profiles/r05_wgrad_kw3.txt), the copies at the ~145 cycles a wave needs to issue one 1 KiB LDS-DMA piece
// (profiles/r05_producer_wave_experiment.txt).
static bool wgrad_kw3(int taps, int cout, int cin, int stride, int ups, bool hp) {
#ifdef LDM_EXPERIMENTS
    static const int on = ldm_xknob("LDM_WGRAD_KW3", 0);
    return on && !hp && taps == 27 && stride == 1 && ups == 0 && cin > 64 && cout > 64;
#else
    return false;
#endif
}
static int wgrad_ksplit(long M, int taps, int cout, int cin, bool hp, int stride, int ups) {
    const int pm = wgrad_pair(taps, cout, cin, stride, ups, hp);
    const bool k3 = wgrad_kw3(taps, cout, cin, stride, ups, hp);
    const long wgs = k3 ? 9L * ((cout + 127) / 128) * ((cin + 63) / 64)
                        : (long)(pm == 3 ? 2 * (taps / 3) : pm == 2 ? taps / 3 : pm == 1 ? (taps + 1) / 2 : taps) * ((cout + 127) / 128) * ((cin + 127) / 128);
    const long steps = (M + 63) / 64;
    // tuning knob: workgroups aimed at (default: one round of 256 CUs; the fp32 kernel, latency bound on its operand loads, wants three per CU: 49.3 -> 46.6 ms per step)
    const long target = ldm_xknob("LDM_WGRAD_WGS", hp ? 768 : 256);
    long k = (target + wgs / 2) / wgs;                       // nearest count of whole rounds
    // at least 16 K steps per workgroup for a 3^3 conv (prologue and ring fill amortised); a 1x1 conv at 12^3 is 27 steps on 4 - 12 workgroups
    // in all (24.7 us of serial K loop, 20 such launches per UNet training step): there 4 steps per workgroup are enough
    const long min_steps = taps == 1 ? 4 : 16;
    if (k > steps / min_steps) k = steps / min_steps;
    // at most 16 copies of a 3^3 weight-sized matrix for the export to fold; a 1x1 conv's matrix is 27 x smaller and its grid is ksplit
    // workgroups in all (nin_shortcut 128 -> 64 over 64^3 voxels: 16 workgroups ran 147 us on 6 % of the chip), so: up to 64 there
    const long cap = taps == 1 ? 64 : pm == 2 ? 32 : 16;     // the three-tap form has 9 workgroups per voxel range (and a 64 x 64 matrix per tap): 28 ranges fill the chip
    if (k > cap) k = cap;
    return (int)(k < 1 ? 1 : k);
}
static int launch_wgrad(const WgradParams& p0, hipStream_t s) {
    WgradParams p = p0;
    const int taps_ = p.ksize * p.ksize * p.ksize;
    p.pair = wgrad_pair(taps_, p.Cout, p.Cin, p.stride, p.ups, false);
    if ((p.pair == 1 || p.pair == 2) && p.cx > 64) p.pair = 0;      // stored channels decide what fits a half row
    if (p.pair == 2 && p.cdy > 64) p.pair = 1;
    if (p.pair == 3 && p.cdy > 64) p.pair = 0;
#ifdef LDM_EXPERIMENTS
    if (p.pair == 0 && wgrad_kw3(taps_, p.Cout, p.Cin, p.stride, p.ups, false) && p.pad == 1 && p.Wout >= 8 && p.Dout == p.Din && p.Hout == p.Hin && p.Wout == p.Win) {
        p.ci_tiles = (p.Cin + 63) / 64;
        static bool attr3_tab[32] = {}; bool& attr3 = attr_flag(attr3_tab);
        if (!attr3) { HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_kw3_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, WG3_LDS)); attr3 = true; }
        { const int dbg = (int)ldm_xknob("LDM_CONV_DBG", 0);  // timing ablations (results are wrong): 4 no copies, 8 no MFMAs, 16 no fragment reads, 32 no masks, 64 no per-step barrier
#define W3_ABL(A) if (dbg == A) { HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_kw3_kernel<A>), hipFuncAttributeMaxDynamicSharedMemorySize, WG3_LDS)); \
          hipLaunchKernelGGL(conv_wgrad_kw3_kernel<A>, dim3(p.co_tiles * p.ci_tiles * 9 * p.ksplit), dim3(512), WG3_LDS, s, p); return 0; }
          W3_ABL(4) W3_ABL(8) W3_ABL(16) W3_ABL(32) W3_ABL(64) W3_ABL(20) W3_ABL(52) W3_ABL(116) W3_ABL(48) W3_ABL(112) W3_ABL(96)
#undef W3_ABL
        }
        if (ldm_xknob("LDM_WGRAD_KW3", 0) == 2) {           // sixteen-wave form
            static bool attr3w_tab[32] = {}; bool& attr3w = attr_flag(attr3w_tab);
            if (!attr3w) { HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_kw3w16_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, WG3_LDS)); attr3w = true; }
            hipLaunchKernelGGL(conv_wgrad_kw3w16_kernel<0>, dim3(p.co_tiles * p.ci_tiles * 9 * p.ksplit), dim3(1024), WG3_LDS, s, p);
            return 0;
        }
        hipLaunchKernelGGL(conv_wgrad_kw3_kernel<0>, dim3(p.co_tiles * p.ci_tiles * 9 * p.ksplit), dim3(512), WG3_LDS, s, p);
        return 0;
    }
#endif
    const int tg_ = p.pair == 3 ? 2 * (taps_ / 3) : p.pair == 2 ? taps_ / 3 : p.pair ? (taps_ + 1) / 2 : taps_;
    constexpr int LDS = 4 * 2 * 64 * 256 + 3 * 256 * 4;        // ring + triple-buffered source-offset table (up to four sections)
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) { HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS)); attr_set = true; }
    { const int dbg = (int)ldm_xknob("LDM_CONV_DBG", 0);      // timing ablations (results are wrong; experiments builds only)
#define W1_ABL(A) if (dbg == A) { HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_kernel<A>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS)); \
          hipLaunchKernelGGL(conv_wgrad_kernel<A>, dim3(p.co_tiles * p.ci_tiles * tg_ * p.ksplit), dim3(512), LDS, s, p); return 0; }
      W1_ABL(4) W1_ABL(8) W1_ABL(16) W1_ABL(12) W1_ABL(20) W1_ABL(24)
#undef W1_ABL
    }
    static const int w16 = ldm_knob("LDM_WGRAD_W16", 1);     // sixteen waves per workgroup where no several-taps form applies (conv_wgrad_w16.h)
    if (w16 && p.pair == 0) {
        static bool attr16_tab[32] = {}; bool& attr16 = attr_flag(attr16_tab);
        if (!attr16) { HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_w16_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS)); attr16 = true; }
        hipLaunchKernelGGL(conv_wgrad_w16_kernel<0>, dim3(p.co_tiles * p.ci_tiles * tg_ * p.ksplit), dim3(1024), LDS, s, p);
        return 0;
    }
    hipLaunchKernelGGL(conv_wgrad_kernel<0>, dim3(p.co_tiles * p.ci_tiles * tg_ * p.ksplit), dim3(512), LDS, s, p);
    return 0;
}

static bool wt_stores() { static const int v = ldm_xknob("LDM_WT_STORES", 1); return v != 0; }   // GroupNorm / finalize outputs written through (sc1): -24 us per step
// gn_fused_apply_kernel over `chunks` row chunks (gn_row_chunks with gn_fused_blocks()) of every 64-channel slice of every sample
// (a template only so that its kernels are instantiated at run_plan's first launch of it: the device code keeps its order)
template <class P> static void launch_gn_fused(P p, int chunks, hipStream_t s) {
    p.xcd_rows = xcd_rows_mode();
    const dim3 grid(chunks, (p.ca + p.cb + 63) / 64, p.N);
    if (wt_stores()) hipLaunchKernelGGL(gn_fused_apply_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gn_fused_apply_kernel<false>, grid, dim3(256), 0, s, p);
}

// ---- the conv family's records (ConvRec) as the kernels' parameter structs
// every integer of a bf16 conv launch, from the record and its configuration: the plans (conv_params) and ldm_op_conv3d* add the operands
static ConvParams conv_params_geom(const ConvRec& c, const ConvCfg& cc) {
    ConvParams p{};
    p.c0a = c.ca; p.c0b = c.cb; p.c1a = c.c1a; p.c1b = c.c1b;
    p.N = c.N; p.Din = c.Din; p.Hin = c.Hin; p.Win = c.Win; p.Dout = c.Dout; p.Hout = c.Hout; p.Wout = c.Wout;
    p.ksize = c.k; p.stride = c.stride; p.pad = c.pad; p.ups = c.ups; p.exact = c.exact; p.M = c.M;
    p.mtiles = conv_mtiles(c, cc); p.ntiles = c.cout_pad / (64 * cc.wgn); p.halo_mtps = cc.mtps; p.q_per_split = cc.qps;
    p.phase_mode = c.phase; p.mtiles_pp = c.phase ? p.mtiles / (8 * c.N) : 0;
    if (c.x3) { p.x3_n = (c.ca / 2) / 64; p.raw_partial = (c.ep32_ndhwc || c.ep32_ncdhw) ? 0 : 1; }   // fp32 precision: 3 x bf16 product on the halo kernel
    p.CoutS = c.couts; p.CoutPad = c.cout_pad; p.CoutReal = c.cout_real; p.nchunk0 = c.nchunk0; p.nchunk1 = c.nchunk1;
    p.steps0 = c.k * c.k * c.k * c.nchunk0; p.steps1 = c.nchunk1;
    p.splitk = cc.splitk; p.steps_per_split = cc.halo ? 3 * cc.qps : (p.steps0 + p.steps1 + p.splitk - 1) / p.splitk;
    p.temb_stride = c.temb_stride; p.slab_lg = cc.slab_lg;
    return p;
}
static ConvParams conv_params(const Op& o, const Bases& bs) {              // OP_CONV, OP_FINALIZE, OP_FIN_GN
    const ConvRec& c = o.cv; ConvParams p = conv_params_geom(c, o.cc);
    p.x0a = (const bf16_t*)rp(bs, c.xa); p.x0b = (const bf16_t*)rp(bs, c.xb); p.w0 = (const bf16_t*)rp(bs, c.w);
    p.x1a = (const bf16_t*)rp(bs, c.x1a); p.x1b = (const bf16_t*)rp(bs, c.x1b); p.w1 = (const bf16_t*)rp(bs, c.w1);
    p.zero_page = (const bf16_t*)bs.p[BASE_W];
    p.bias = (const float*)rp(bs, c.bias); p.bias2 = (const float*)rp(bs, c.bias2); p.temb = (const float*)rp(bs, c.temb);
    if (c.ep32_ndhwc) { p.out32 = (float*)rp(bs, c.out); p.residual32 = (const float*)rp(bs, c.residual); }   // ... with the epilogue fused (splitk 1): fp32 output and residual
    else {
        p.residual = (const bf16_t*)rp(bs, c.residual);
        if (c.f32_out) p.out_f32 = (float*)rp(bs, c.out); else p.out = (bf16_t*)rp(bs, c.out);
    }
    p.partial = (float*)rp(bs, c.partial); p.stats = (float*)rp(bs, c.stats);
    return p;
}
static Conv32Params conv32_params(const Op& o, const Bases& bs) {          // OP_CONV32, OP_FIN32
    const ConvRec& c = o.cv; Conv32Params p{};
    p.xa = (const float*)rp(bs, c.xa); p.xb = (const float*)rp(bs, c.xb); p.ca = c.ca; p.cb = c.cb; p.w = (const float*)rp(bs, c.w);
    p.N = c.N; p.Din = c.Din; p.Hin = c.Hin; p.Win = c.Win; p.Dout = c.Dout; p.Hout = c.Hout; p.Wout = c.Wout;
    p.ksize = c.k; p.stride = c.stride; p.pad = c.pad; p.ups = c.ups; p.exact = c.exact; p.M = c.M;
    p.CoutS = c.couts; p.CoutPad = c.cout_pad; p.CoutReal = c.cout_real; p.nchunk = c.nchunk0; p.steps = c.k * c.k * c.k * c.nchunk0;
    p.splitk = o.cc.splitk; p.steps_per_split = (p.steps + p.splitk - 1) / p.splitk; p.mtiles = c.mtiles; p.ntiles = c.ntiles;
    p.bias = (const float*)rp(bs, c.bias); p.temb = (const float*)rp(bs, c.temb); p.temb_stride = c.temb_stride; p.residual = (const float*)rp(bs, c.residual);
    if (c.f32_out) p.out_ncdhw = (float*)rp(bs, c.out); else p.out = (float*)rp(bs, c.out);
    p.partial = (float*)rp(bs, c.partial);
    if (c.stats_nrb > 0) { p.stats = (float*)rp(bs, c.stats); p.stats_nrb = c.stats_nrb; p.stats_rows = c.stats_rows; }
    return p;
}
static FinalizeParams finalize_params(const ConvParams& p) {                // the split-K finalize of the conv that ran with p
    FinalizeParams f{}; f.partial = p.partial; f.splitk = p.splitk; f.M = p.M; f.CoutPad = p.CoutPad; f.CoutS = p.CoutS; f.CoutReal = p.CoutReal;
    f.DHWo = p.Dout * p.Hout * p.Wout; f.bias = p.bias; f.bias2 = p.bias2; f.temb = p.temb; f.temb_stride = p.temb_stride; f.residual = p.residual;
    f.out = p.out; f.out_f32 = p.out_f32; f.stats = p.stats;
    return f;
}
template <class P> static P wgrad_params(const WgradRec& w, const Bases& bs) {   // OP_WGRAD as WgradParams or Wgrad32Params
    P p{}; p.dy = (decltype(p.dy))rp(bs, w.dy); p.cdy = w.cdy; p.x = (decltype(p.x))rp(bs, w.x); p.cx = w.cx;
    p.dw = (float*)rp(bs, w.dw); p.Cout = w.Cout; p.Cin = w.Cin; p.dw_ld = w.dw_ld; p.dw_ci_off = w.dw_ci_off;
    p.N = w.N; p.Din = w.Din; p.Hin = w.Hin; p.Win = w.Win; p.Dout = w.Dout; p.Hout = w.Hout; p.Wout = w.Wout;
    p.ksize = w.ksize; p.stride = w.stride; p.pad = w.pad; p.ups = w.ups; p.M = w.M;
    p.co_tiles = (p.Cout + 127) / 128; p.ci_tiles = (p.Cin + 127) / 128; p.ksplit = w.ksplit;
    p.slab_stride = (long)w.ksize * w.ksize * w.ksize * w.rows_total * w.dw_ld;
    return p;
}
template <class P> static P attn_params(const AttnRec& a, const Bases& bs) {       // OP_ATTN as AttnParams, OP_ATTN32 as Attn32Params
    P p{}; p.qkv = (decltype(p.qkv))rp(bs, a.qkv); p.out = (decltype(p.out))rp(bs, a.out); p.lse = (float*)rp(bs, a.lse);
    p.B = a.B; p.N = a.N; p.C = a.C; p.heads = a.heads; p.d = a.d; p.scale = a.scale;
    return p;
}
template <class P> static P attn_bwd_params(const AttnRec& a, const Bases& bs) {   // OP_ATTN_BWD as AttnBwdParams or Attn32BwdParams
    P p{}; p.qkv = (decltype(p.qkv))rp(bs, a.qkv); p.o = (decltype(p.o))rp(bs, a.out); p.d_o = (decltype(p.d_o))rp(bs, a.d_o);
    p.lse = (const float*)rp(bs, a.lse); p.delta = (float*)rp(bs, a.delta); p.dqkv = (decltype(p.dqkv))rp(bs, a.dqkv);
    p.B = a.B; p.N = a.N; p.C = a.C; p.d = a.d; p.heads = a.heads; p.scale = a.scale;
    return p;
}

// per-op timeline of every launch plan that runs while it is on (ldm_set_plan_trace; initial state from LDM_PLAN_TRACE)
struct PlanTrace { bool on = false; std::string path; PlanTrace() { const char* e = getenv("LDM_PLAN_TRACE"); if (e && *e) { on = true; path = e; } } };
static PlanTrace g_plan_trace;
struct LaneCtx { GradSyncState* sync = nullptr;      // the gradient exchange of the backward plans (comm stream, events)
                 float* acc = nullptr; int acc_assign = 0; float acc_scale = 1.f; };   // accumulation over micro-batches (null: off)
// what a training backward with a gradient buffer runs at its OP_BUCKET / OP_BUCKET_JOIN ops: the accumulate pass if armed, and the exchange
// if a communicator is attached -- with accumulation only on the last micro-batch of a window (on the others nothing is begun, issued or joined)
static int backward_lanes(ldm_model* m, hipStream_t s, LaneCtx* lanes);
// classifier-free guidance: the launches of the guided kernels (norm_elem.h), defined behind every other launch, at the end of this file
static void guided_layout_launch(OpKind kind, const LayoutRec& l, const float* x, int cx, const float* cond, int cc, float fill, void* dst, hipStream_t s);
static void guided_combine_launch(const float* u, const float* c, float w, float* out, int64_t n, hipStream_t s);

static int run_plan(const Plan& plan, const Bases& bs, const int* rt, hipStream_t s, size_t begin = 0, size_t end = (size_t)-1,
                    LaneCtx lanes = LaneCtx()) {
    if (end > plan.ops.size()) end = plan.ops.size();
    // LDM_PLAN_TRACE=<file>: measurement aid (tools/plan_trace.py) -- a HIP event before every op, one CSV row per op appended
    const char* trace_path = g_plan_trace.on ? g_plan_trace.path.c_str() : nullptr;
    std::vector<hipEvent_t> tev;
    if (trace_path) { tev.resize(end - begin + 1); for (auto& e : tev) HIP_TRY(hipEventCreate(&e)); }
    struct TraceDone {
        const Plan& plan; size_t begin, end; std::vector<hipEvent_t>& ev; hipStream_t s; const char* path;
        ~TraceDone() {
            if (ev.empty()) return;
            (void)hipEventRecord(ev.back(), s); (void)hipEventSynchronize(ev.back());
            FILE* f = fopen(path, "a");
            for (size_t oi = begin; oi < end && f; ++oi) {
                const Op& o = plan.ops[oi]; float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[oi - begin], ev[oi - begin + 1]);
                fprintf(f, "%zu,%zu,%d,%.3f", plan.ops.size(), oi, (int)o.kind, ms * 1e3f);
                const ConvRec& c = o.cv;
                if (o.kind == OP_CONV || o.kind == OP_FINALIZE)     // ups= prints the addressing flags as one bit set, as it always has
                    fprintf(f, ",M=%d k=%d s=%d ups=%d cin=%d+%d(x%d) cin1=%d couts=%d cfg=%dx%dx%d splitk=%d halo=%d mtps=%d qps=%d cube=%d", c.M, c.k, c.stride,
                            c.ups | c.exact << 1 | c.phase << 2 | c.x3 << 3 | c.ep32_ndhwc << 4 | c.ep32_ncdhw << 5, c.ca, c.cb, c.nchunk0, c.c1a + c.c1b, c.couts,
                            o.cc.wgm, o.cc.wgn, o.cc.bk, o.cc.splitk, o.cc.plane ? 6 : o.cc.halo, o.cc.mtps, o.cc.qps, o.cc.cube);   // plane: halo code 6, as ldm_model_plan_conv_cfgs
                else {                                              // every other kind: six integers, those its record began with before it had names
                    const GnRec& g = o.gn; const WgradRec& w = o.wg; const LayoutRec& l = o.lay; const AttnRec& at = o.at;
                    const LinRec& li = o.lin; const ElemRec& el = o.el; const RangeRec& r = o.rg;
                    int v[6] = {};
                    auto six = [&](int a, int b, int c2, int d, int e, int h) { v[0] = a; v[1] = b; v[2] = c2; v[3] = d; v[4] = e; v[5] = h; };
                    switch (o.kind) {
                        case OP_FIN_GN: six(c.gn_groups, c.gn_silu, c.gn_lg, c.c1b, c.N, c.Din); break;
                        case OP_CONV32: case OP_FIN32: six(c.ca, c.cb, c.stats_nrb, c.stats_rows, c.N, c.Din); break;
                        case OP_CONV_THIN: six(c.N, c.Din, c.Hin, c.Win, c.x3 ? c.ca / 2 * 3 : c.ca, c.cout_pad); break;
                        case OP_CONV_BLOCK: six(c.N, c.Dout, c.Hout, c.Wout, c.ca, o.cc.th); break;
                        case OP_DGRAD_THIN_PACK: six(c.ca, c.couts, c.cout_real, c.cout_pad, c.cb, c.x3); break;
                        case OP_DGRAD_UNPACK: six(l.N, l.c_real, l.c_stored, l.DHW, l.esz, 0); break;
                        case OP_DGRAD_THIN: six(c.N, c.Din, c.Hin, c.Win, c.x3 ? 3 * c.ca : c.ca, c.cout_real); break;
                        case OP_GEMM_LIGHT: case OP_GEMM_LIGHT32: six(c.M, c.ca + c.cb, c.couts, c.cout_pad, o.cc.big, c.ca); break;
                        case OP_GN_STATS: case OP_GN_STATS32: six(g.ca, g.cb, g.DHW, g.nslab, g.rows_per_slab, g.N); break;
                        case OP_GN_FINALIZE: six(g.nslab, g.ca + g.cb, g.groups, g.DHW, g.N, 0); break;
                        case OP_GN_PREP: six(g.ca, g.cb, g.nrb_a, g.groups, g.DHW, g.N); break;
                        case OP_GN_FUSED: six(g.ca, g.cb, g.nrb_a, g.nrb_b, g.groups, g.DHW); break;
                        case OP_GN_APPLY: six(g.ca, g.cb, g.DHW, g.N, g.silu, 0); break;
                        case OP_GN_APPLY32: six(g.ca, g.cb, g.DHW, g.N, g.silu, g.nrb_a ? 1 : g.nslab); break;   // (the producer-partials form always printed 1)
                        case OP_COLSUM: six(g.N, g.nslab, g.ca, g.over_n, g.count, g.out_stride); break;
                        case OP_GNB: six(g.ca, g.cb, g.groups, g.DHW, g.N, g.silu); break;
                        case OP_WGRAD: six(w.cdy, w.cx, w.Cout, w.Cin, w.dw_ld, w.dw_ci_off); break;
                        case OP_PACK: case OP_PACK32: six(l.N, l.c_real, l.c_stored, l.DHW, l.internal, 0); break;
                        case OP_IM2COL: six(l.N, l.c_real, l.c_stored, l.D, l.H, l.W); break;
                        case OP_UPS_SPLIT32: six(l.N, l.c_stored, l.D, l.H, l.W, l.ups); break;
                        case OP_TAP: six(l.N, l.c_real, l.c_stored, l.DHW, l.esz, l.mode); break;
                        case OP_ATTN: case OP_ATTN32: six(at.B, at.N, at.C, at.heads, at.d, at.x3); break;
                        case OP_ATTN_BWD: six(at.B, at.N, at.C, at.d, at.fp32, 0); break;
                        case OP_SINUSOID: six(li.B, li.O, 0, 0, 0, 0); break;
                        case OP_TEMB_ROW: six(li.O, li.B, 0, 0, 0, 0); break;
                        case OP_GEMV: case OP_GEMV32: six(li.I, li.O, li.x_stride, li.y_stride, li.silu, li.B); break;
                        case OP_LIN_DX: case OP_LIN_DW: six(li.B, li.I, li.O, li.dy_stride, li.x_stride, li.silu); break;
                        case OP_VAE_HEADS: six(el.N, el.L, el.DHW, 0, 0, 0); break;
                        case OP_VAE_HEADS_BWD: six(el.N, el.L, el.C, el.DHW, el.c_dz, el.fp32); break;
                        case OP_ADD: six(el.n, el.fp32, 0, 0, 0, 0); break;
                        case OP_SUMPOOL: six(el.N, el.D, el.H, el.W, el.C, el.fp32); break;
                        case OP_WT_BATCH: six(r.fp32, 0, 0, 0, 0, 0); break;
                        case OP_COLSUM_BATCH: case OP_EXPORT_BATCH: six(r.first, r.end, 0, 0, 0, 0); break;
                        case OP_BUCKET: six(r.first, r.count, 0, 0, 0, 0); break;
                        case OP_BUCKET_JOIN: case OP_WT: case OP_EXPORT: case OP_CONV: case OP_FINALIZE: break;   // six zeros; the conv rows are printed above
                    }
                    fprintf(f, ",i=%d %d %d %d %d %d", v[0], v[1], v[2], v[3], v[4], v[5]);
                }
                fprintf(f, "\n");
            }
            if (f) fclose(f);
            for (auto e : ev) (void)hipEventDestroy(e);
        }
    } trace_done{plan, begin, end, tev, s, trace_path};
    for (size_t oi = begin; oi < end; ++oi) {
        const Op& o = plan.ops[oi];
        if (trace_path) HIP_TRY(hipEventRecord(tev[oi - begin], s));
        switch (o.kind) {
            case OP_PACK: case OP_PACK32: case OP_IM2COL: {
                // two fp32 NCDHW sources (x | cond) -> one zero-padded NDHWC tensor (bf16 | fp32), or the first conv's bf16 patch matrix
                const LayoutRec& l = o.lay;
                int cx = rt[0], cc = rt[1];
                if (l.internal) { cx = l.c_real; cc = 0; }   // fixed channel count, single source
                if (cx + cc != l.c_real) return fail(LDM_ERR_BAD_ARG, "x_channels + cond_channels = %d, model expects %d", cx + cc, l.c_real);
                const float* xa = (const float*)rp(bs, l.a); const float* xb = (const float*)rp(bs, l.b);
                if (l.guided) {                                 // N = 2 B samples from the caller's B: (x | fill) first, (x | cond) second
                    if (cc < 1 || !xb || (l.N & 1)) return fail(LDM_ERR_BAD_ARG, "a guided plan needs a condition tensor");
                    guided_layout_launch(o.kind, l, xa, cx, xb, cc, bs.guide_fill, rp(bs, l.dst), s);
                } else
                if (o.kind == OP_IM2COL) launch_pack_im2col(xa, cx, xb, cc, (bf16_t*)rp(bs, l.dst), l.N, l.D, l.H, l.W, l.c_stored, s);
                else launch_pack2(xa, cx, xb, cc, rp(bs, l.dst), l.N, l.c_stored, l.DHW, o.kind == OP_PACK32, s);
                break; }
            case OP_CONV_THIN: {
                const ConvRec& c = o.cv;
                ThinParams q{}; q.x = (const bf16_t*)rp(bs, c.xa); q.w = (const bf16_t*)rp(bs, c.w); q.bias = (const float*)rp(bs, c.bias);
                q.out = (float*)rp(bs, c.out); q.N = c.N; q.D = c.Din; q.H = c.Hin; q.W = c.Win; q.CoutPad = c.cout_pad; q.CoutReal = c.cout_real;
                if (c.x3) { q.x3_c = c.ca / 2; q.Cin = 3 * q.x3_c; } else q.Cin = c.ca;   // x3: K runs over [hi | lo | hi]
                if (!q.w) return fail(LDM_ERR_NOT_LOADED, "the weight arena is empty");
                HIP_TRY(launch_conv_thin(q, s));
                break; }
            case OP_DGRAD_THIN_PACK: {  // conv_in's packed [27][cout_pad][cin_s] weights (bf16, or the fp32 arena's) -> [27 mirrored taps][32][K]
                const ConvRec& c = o.cv;
                const char* w = rp(bs, c.w);
                if (!w) return fail(LDM_ERR_NOT_LOADED, c.x3 ? "fp32 precision: the fp32 weight arena is empty" : "the weight arena is empty");
                launch_dgrad_thin_pack(w, c.x3, (bf16_t*)rp(bs, c.out), c.couts, c.cout_real, c.x3 ? 3 * c.ca : c.ca, c.x3, c.cb, 1, (long)c.cout_pad * c.cb, s);
                break; }
            case OP_DGRAD_THIN: {       // bs[IO1] = dx, bs[IO2] = dcond (either may be null), in_cx + in_cc = the conv's real input channels
                const ConvRec& c = o.cv;
                if (bs.in_cx + bs.in_cc != c.cout_real || bs.in_cx < 0 || bs.in_cc < 0)
                    return fail(LDM_ERR_BAD_ARG, "x_channels + cond_channels = %d, model expects %d", bs.in_cx + bs.in_cc, c.cout_real);
                dgrad_thin_launch((const bf16_t*)rp(bs, c.xa), (const bf16_t*)rp(bs, c.w), (float*)bs.p[BASE_IO1], (float*)bs.p[BASE_IO2], bs.in_cx, bs.in_cc,
                                  c.N, c.Din, c.Hin, c.Win, c.x3 ? 3 * c.ca : c.ca, c.x3 ? c.ca : 0, s);
                break; }
            case OP_DGRAD_UNPACK: {     // bs[IO1] = dx, bs[IO2] = dcond (either may be null): channels [0, cx) and [cx, cx + cc) of the NDHWC gradient
                const LayoutRec& l = o.lay;
                if (bs.in_cx + bs.in_cc != l.c_real || bs.in_cx < 0 || bs.in_cc < 0)
                    return fail(LDM_ERR_BAD_ARG, "x_channels + cond_channels = %d, model expects %d", bs.in_cx + bs.in_cc, l.c_real);
                float* dst[2] = {(float*)bs.p[BASE_IO1], (float*)bs.p[BASE_IO2]};
                const int c0[2] = {0, bs.in_cx}, cn[2] = {bs.in_cx, bs.in_cc};
                for (int k = 0; k < 2; ++k) {
                    if (!dst[k] || cn[k] < 1) continue;
                    const dim3 grid(grid_for((long)l.N * cn[k] * l.DHW));
                    if (l.esz == 4) hipLaunchKernelGGL(tap_export_kernel<float>, grid, dim3(256), 0, s, (const float*)rp(bs, l.a) + c0[k], dst[k], l.N, cn[k], l.c_stored, l.DHW);
                    else hipLaunchKernelGGL(tap_export_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)rp(bs, l.a) + c0[k], dst[k], l.N, cn[k], l.c_stored, l.DHW);
                }
                break; }
            case OP_CONV_BLOCK: {
                const ConvRec& c = o.cv;
                BlockParams q{}; q.x = (const bf16_t*)rp(bs, c.xa); q.w = (const bf16_t*)rp(bs, c.w); q.bias = (const float*)rp(bs, c.bias);
                q.temb = (const float*)rp(bs, c.temb); q.temb_stride = c.temb_stride; q.residual = (const bf16_t*)rp(bs, c.residual); q.out = (bf16_t*)rp(bs, c.out);
                q.stats = (float*)rp(bs, c.stats); q.N = c.N; q.D = c.Dout; q.H = c.Hout; q.W = c.Wout; q.Cin = c.ca;
                if (!q.w) return fail(LDM_ERR_NOT_LOADED, "the weight arena is empty");
                if (c.couts == 128) HIP_TRY(launch_conv_block128(q, s)); else HIP_TRY(launch_conv_block(q, o.cc.th, s));
                break; }
            case OP_UPS_SPLIT32: {      // N, C, D, H, W of the source, upsample (1) or same size (0)
                const LayoutRec& l = o.lay;
                launch_split_f32((const float*)rp(bs, l.a), (bf16_t*)rp(bs, l.dst), l.N, l.c_stored, l.D, l.H, l.W, l.ups, s);
                break; }
            case OP_CONV32: case OP_FIN32: {
                const Conv32Params p = conv32_params(o, bs);
                if (!p.w) return fail(LDM_ERR_NOT_LOADED, "fp32 precision: the fp32 weight arena is empty (re-upload the parameters after ldm_model_set_precision)");
                if (o.kind == OP_CONV32) launch_conv32(p, o.cc.bk == 32, o.cc.wgn * 64, s);
                else launch_fin32(p, s);
                break; }
            case OP_GEMM_LIGHT32: {
                const ConvRec& c = o.cv;
                LightX3Params p{};
                p.x = (const float*)rp(bs, c.xa); p.xb = (const float*)rp(bs, c.xb); p.ca = c.ca;
                p.w = (const float*)rp(bs, c.w);
                if (!p.w) return fail(LDM_ERR_NOT_LOADED, "fp32 precision: the fp32 weight arena is empty (re-upload the parameters after ldm_model_set_precision)");
                p.bias = (const float*)rp(bs, c.bias); p.residual = (const float*)rp(bs, c.residual);
                p.out = (float*)rp(bs, c.out); p.stats = (float*)rp(bs, c.stats);
                p.M = c.M; p.K = c.ca + c.cb; p.CoutS = c.couts;
                HIP_TRY(launch_gemm_light_x3(p, c.cout_pad, o.cc.big, s));
                break; }
            case OP_GN_STATS32: {
                const GnRec& g = o.gn;
                Gn32Params p{}; p.xa = (const float*)rp(bs, g.xa); p.xb = (const float*)rp(bs, g.xb); p.ca = g.ca; p.cb = g.cb;
                p.DHW = g.DHW; p.nslab = g.nslab; p.rows_per_slab = g.rows_per_slab; p.N = g.N; p.partial = (float*)rp(bs, g.partial);
                hipLaunchKernelGGL(gn_stats_f32_kernel, dim3(g.nslab, g.N), dim3(256), 0, s, p);
                break; }
            case OP_GN_APPLY32: {
                const GnRec& g = o.gn;
                if (g.nrb_a || g.nslab) {    // statistics fold + apply in one launch (inference plans)
                    Gn32FusedParams q{}; q.xa = (const float*)rp(bs, g.xa); q.xb = (const float*)rp(bs, g.xb); q.ca = g.ca; q.cb = g.cb;
                    q.DHW = g.DHW; q.N = g.N; q.silu = g.silu; q.groups = g.groups; q.rows_per_block = g.rows_per_block; q.eps = g.eps;
                    q.gamma = (const float*)rp(bs, g.gamma); q.beta = (const float*)rp(bs, g.beta);
                    if (g.nrb_a) {           // the producers' partials (the kernel does not read nslab then; 1 is what this launch has always carried)
                        q.sa = (const float*)rp(bs, g.stats_a); q.sb = (const float*)rp(bs, g.stats_b); q.nrb_a = g.nrb_a; q.nrb_b = g.nrb_b; q.nslab = 1;
                    } else { q.partial = (const float*)rp(bs, g.partial); q.nslab = g.nslab; }
                    if (g.out_hl) q.out_hl = (bf16_t*)rp(bs, g.out); else q.out = (float*)rp(bs, g.out);
                    hipLaunchKernelGGL(gn32_fold_apply_kernel, dim3(g.chunks, (g.ca + g.cb + 63) / 64, g.N), dim3(256), 0, s, q);
                } else {
                    Gn32Params p{}; p.xa = (const float*)rp(bs, g.xa); p.xb = (const float*)rp(bs, g.xb); p.ca = g.ca; p.cb = g.cb;
                    p.DHW = g.DHW; p.N = g.N; p.silu = g.silu; p.ab = (const float*)rp(bs, g.ab); p.out = (float*)rp(bs, g.out);
                    hipLaunchKernelGGL(gn_apply_f32_kernel, dim3(grid_for((long)g.N * g.DHW * ((g.ca + g.cb) / 4), 256, 4096)), dim3(256), 0, s, p);
                }
                break; }
            case OP_ATTN32: {
                Attn32Params p = attn_params<Attn32Params>(o.at, bs); p.x3 = o.at.x3;
                HIP_TRY(launch_attn_f32(p, s));
                break; }
            case OP_GEMV: case OP_GEMV32: {
                const LinRec& l = o.lin;
                const char* w = rp(bs, l.w); const float* bias = (const float*)rp(bs, l.bias); const float* x = (const float*)rp(bs, l.x);
                if (o.kind == OP_GEMV32 && !w) return fail(LDM_ERR_NOT_LOADED, "fp32 precision: the fp32 weight arena is empty");
                launch_gemv(w, o.kind == OP_GEMV32, bias, x, (float*)rp(bs, l.y), l.B, l.I, l.O, l.x_stride, l.y_stride, l.silu, s);
                break; }
            case OP_TAP: {
                const LayoutRec& l = o.lay;
                float* dst = (float*)rp(bs, l.dst); const float* src = (const float*)rp(bs, l.b);
                const long total = (long)l.N * l.c_real * l.DHW;
                if (dst) {
                    if (l.esz == 4) hipLaunchKernelGGL(tap_export_kernel<float>, dim3(grid_for(total)), dim3(256), 0, s, (const float*)rp(bs, l.a), dst, l.N, l.c_real, l.c_stored, l.DHW);
                    else hipLaunchKernelGGL(tap_export_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, s, (const bf16_t*)rp(bs, l.a), dst, l.N, l.c_real, l.c_stored, l.DHW);
                }
                if (src && l.mode == 2) {
                    launch_pack2(src, l.c_real, nullptr, 0, rp(bs, l.a), l.N, l.c_stored, l.DHW, l.esz == 4, s);
                }
                break; }
            case OP_FIN_GN: {            // an OP_FINALIZE that also applies the GroupNorm(+SiLU) reading it
                const ConvRec& c = o.cv;
                FinGnParams q{}; q.f = finalize_params(conv_params(o, bs));
                q.gamma = (const float*)rp(bs, c.gamma); q.beta = (const float*)rp(bs, c.beta); q.y = (bf16_t*)rp(bs, c.gn_out);
                q.groups = c.gn_groups; q.silu = c.gn_silu; q.lg = c.gn_lg; q.eps = c.gn_eps;
                HIP_TRY(launch_fin_gn(q, c.N, wt_stores(), s));
                break; }
            case OP_CONV: case OP_FINALIZE: {
                const ConvParams p = conv_params(o, bs);
                if (o.kind == OP_CONV) { LDM_TRY(launch_conv(p, o.cc, s)); }
                else launch_finalize(finalize_params(p), wt_stores(), s);
                break; }
            case OP_GEMM_LIGHT: {
                const ConvRec& c = o.cv;
                LightParams p{}; p.x = (const bf16_t*)rp(bs, c.xa); p.w = (const bf16_t*)rp(bs, c.w); p.bias = (const float*)rp(bs, c.bias);
                p.residual = (const bf16_t*)rp(bs, c.residual); p.out = (bf16_t*)rp(bs, c.out); p.stats = (float*)rp(bs, c.stats);
                p.M = c.M; p.K = c.ca + c.cb; p.CoutS = c.couts; p.xb = (const bf16_t*)rp(bs, c.xb); p.ca = c.ca;
                if (o.cc.wg == 2) {
                    WgGnParams g{}; g.slabs = (const float*)rp(bs, c.gn_stats); g.gamma = (const float*)rp(bs, c.gamma); g.beta = (const float*)rp(bs, c.beta);
                    g.nrb = c.gn_nrb; g.groups = c.gn_groups; g.DHW = c.Dout * c.Hout * c.Wout; g.eps = c.gn_eps;
                    HIP_TRY(launch_gemm_wg(p, c.cout_pad, o.cc.big, s, &g));
                } else
                    HIP_TRY(launch_gemm_1x1(p, c.cout_pad, o.cc.big, o.cc.wg, s));
                break; }
            case OP_GN_STATS: {
                const GnRec& g = o.gn;
                GnStatsParams p{}; p.xa = (const bf16_t*)rp(bs, g.xa); p.xb = (const bf16_t*)rp(bs, g.xb); p.ca = g.ca; p.cb = g.cb;
                p.DHW = g.DHW; p.nslab = g.nslab; p.rows_per_slab = g.rows_per_slab; p.partial = (float*)rp(bs, g.partial);
                hipLaunchKernelGGL(gn_stats_kernel, dim3(g.nslab, g.N), dim3(256), 0, s, p);
                break; }
            case OP_GN_FINALIZE: {
                const GnRec& g = o.gn;
                GnFinalizeParams p{}; p.partial = (const float*)rp(bs, g.partial); p.nslab = g.nslab; p.C = p.Creal = g.ca + g.cb; p.groups = g.groups;
                p.DHW = g.DHW; p.eps = g.eps; p.gamma = (const float*)rp(bs, g.gamma); p.beta = (const float*)rp(bs, g.beta);
                p.ab = (float*)rp(bs, g.ab); p.mr = (float*)rp(bs, g.mr);
                hipLaunchKernelGGL(gn_finalize_kernel, dim3(g.groups, g.N), dim3(256), 0, s, p);
                break; }
            case OP_GN_PREP: {
                const GnRec& g = o.gn;
                GnPrepParams p{}; p.sa = (const float*)rp(bs, g.stats_a); p.sb = (const float*)rp(bs, g.stats_b); p.ca = g.ca; p.cb = g.cb;
                p.nrb_a = g.nrb_a; p.nrb_b = g.nrb_b; p.groups = g.groups; p.DHW = g.DHW; p.eps = g.eps;
                p.gamma = (const float*)rp(bs, g.gamma); p.beta = (const float*)rp(bs, g.beta); p.ab = (float*)rp(bs, g.ab); p.mr = (float*)rp(bs, g.mr);
                hipLaunchKernelGGL(gn_prep_kernel, dim3(g.groups, g.N), dim3(256), 0, s, p);
                break; }
            case OP_GN_FUSED: {
                const GnRec& g = o.gn;
                GnFusedParams p{}; p.xa = (const bf16_t*)rp(bs, g.xa); p.xb = (const bf16_t*)rp(bs, g.xb); p.ca = g.ca; p.cb = g.cb;
                p.sa = (const float*)rp(bs, g.stats_a); p.sb = (const float*)rp(bs, g.stats_b); p.nrb_a = g.nrb_a; p.nrb_b = g.nrb_b;
                p.groups = g.groups; p.DHW = g.DHW; p.N = g.N; p.silu = g.silu; p.rows_per_block = g.rows_per_block; p.eps = g.eps;
                p.gamma = (const float*)rp(bs, g.gamma); p.beta = (const float*)rp(bs, g.beta); p.out = (bf16_t*)rp(bs, g.out);
                p.ab = (float*)rp(bs, g.ab); p.mr = (float*)rp(bs, g.mr);
                launch_gn_fused(p, g.chunks, s);
                break; }
            case OP_GN_APPLY: {
                const GnRec& g = o.gn;
                GnApplyParams p{}; p.xa = (const bf16_t*)rp(bs, g.xa); p.xb = (const bf16_t*)rp(bs, g.xb); p.ca = g.ca; p.cb = g.cb;
                p.DHW = g.DHW; p.N = g.N; p.silu = g.silu; p.ab = (const float*)rp(bs, g.ab); p.out = (bf16_t*)rp(bs, g.out);
                const long total = (long)g.N * g.DHW * ((g.ca + g.cb) / 8);
                hipLaunchKernelGGL(gn_apply_kernel, dim3(grid_for(total, 256, 2048)), dim3(256), 0, s, p);
                break; }
            case OP_ATTN: {
                const AttnParams p = attn_params<AttnParams>(o.at, bs);
                HIP_TRY(launch_attn_fwd(p, s));
                break; }
            case OP_TEMB_ROW: {         // bs[TTAB] = table, bs[SST] = sampler state
                const float* tab = (const float*)bs.p[BASE_TTAB]; const SamplerState* st = (const SamplerState*)bs.p[BASE_SST];
                if (!tab || !st || bs.sampler_steps < 1) return fail(LDM_ERR_BAD_ARG, "denoise-step plan without a sampler / time-embedding table");
                hipLaunchKernelGGL(temb_row_kernel, dim3((o.lin.O / 4 + 255) / 256, o.lin.B), dim3(256), 0, s, tab, st, (float*)rp(bs, o.lin.y), o.lin.O, o.lin.O, bs.sampler_steps);
                break; }
            case OP_SINUSOID:
                launch_sinusoid((const float*)rp(bs, o.lin.x), (float*)rp(bs, o.lin.y), o.lin.B, o.lin.O, s);
                break;
            case OP_VAE_HEADS: {
                const ElemRec& e = o.el;
                launch_vae_heads((const float*)rp(bs, e.ml), (const float*)rp(bs, e.noise), (float*)rp(bs, e.mu), (float*)rp(bs, e.sigma),
                                 (float*)rp(bs, e.z), e.N, e.L, e.DHW, s);
                break; }
            // ------------------------------------------------------------------ backward ops
            case OP_WT: case OP_EXPORT: break;   // unused: every plan uses the batched tables (listed so that -Wswitch keeps reporting a forgotten kind)
            case OP_WT_BATCH:
                if (plan.wt_tab.nblocks && o.rg.fp32) {
                    if (!bs.p[BASE_W32]) return fail(LDM_ERR_NOT_LOADED, "fp32 precision: the fp32 weight arena is empty");
                    hipLaunchKernelGGL(weight_flip_transpose_batched_f32_kernel, dim3(plan.wt_tab.nblocks), dim3(256), 0, s,
                                       (const WtDesc*)plan.wt_tab.descs, (const int2*)plan.wt_tab.map, (const char*)bs.p[BASE_W32], bs.p[BASE_WS]);
                } else if (plan.wt_tab.nblocks)
                    launch_wt_batched((const WtDesc*)plan.wt_tab.descs, (const int2*)plan.wt_tab.map, plan.wt_tab.nblocks, (const char*)bs.p[BASE_W],
                                      (char*)bs.p[BASE_WS], s);
                break;
            case OP_COLSUM_BATCH:
                if (o.rg.end > o.rg.first)
                    launch_colsum_batched((const ColsumDesc*)plan.cs_tab.descs, (const int2*)plan.cs_tab.map + o.rg.first, o.rg.end - o.rg.first, (char*)bs.p[BASE_WS], s);
                break;
            case OP_EXPORT_BATCH:
                if (!bs.p[BASE_IO4]) return fail(LDM_ERR_BAD_ARG, "backward without a gradient buffer");
                if (o.rg.end > o.rg.first)
                    launch_export_batched((const ExportDesc*)plan.exp_tab.descs, (const int2*)plan.exp_tab.map + o.rg.first, o.rg.end - o.rg.first,
                                          (const char*)bs.p[BASE_WS], (float*)bs.p[BASE_IO4], s);
                break;
            case OP_BUCKET: {           // a final tail range of the flat gradient buffer
                float* range = (float*)bs.p[BASE_IO4] + o.rg.first;
                if (lanes.acc) {        // fold it into the accumulator; the exchange (last micro-batch) then carries the accumulated range
                    if (!bs.p[BASE_IO4]) return fail(LDM_ERR_BAD_ARG, "backward without a gradient buffer");
                    LDM_TRY(grad_accum_launch(lanes.acc + o.rg.first, range, o.rg.count, lanes.acc_scale, lanes.acc_assign, s));
                    range = lanes.acc + o.rg.first;
                }
                if (lanes.sync) LDM_TRY(grad_sync_bucket(*lanes.sync, range, o.rg.count, s));
                break;
            }
            case OP_BUCKET_JOIN:
                if (lanes.sync) LDM_TRY(grad_sync_join(*lanes.sync, s));
                break;
            case OP_WGRAD: {
                if (o.wg.fp32) { launch_wgrad32(wgrad_params<Wgrad32Params>(o.wg, bs), s); break; }
                const WgradParams p = wgrad_params<WgradParams>(o.wg, bs);
                if ((long)p.M * p.cdy * 2 >= (1L << 32) || (long)p.N * p.Din * p.Hin * p.Win * p.cx * 2 >= (1L << 32))
                    return fail(LDM_ERR_UNSUPPORTED, "weight gradient: tensor exceeds 4 GiB");
                LDM_TRY(launch_wgrad(p, s));
                break; }
            case OP_COLSUM: {
                const GnRec& g = o.gn;
                launch_colsum((const float*)rp(bs, g.partial), (float*)rp(bs, g.out), g.N, g.nslab, g.ca, g.over_n, g.count, g.out_stride, s);
                break; }
            case OP_GNB: {
                const GnRec& g = o.gn;
                float* flat = (float*)bs.p[BASE_IO4]; float* sink = (float*)rp(bs, g.sink);
                if (!flat && !sink) return fail(LDM_ERR_BAD_ARG, "backward without a gradient buffer");
                float* dgamma = sink ? sink : flat + g.dgamma_flat; float* dbeta = sink ? sink + g.ca + g.cb : flat + g.dbeta_flat;
                // the fold form does not use the group sums; its launches have always carried the column-sum block in their place
                float* gsum = (float*)rp(bs, g.leaves_colsums ? g.cs : g.gsum);
                // what the bf16 and the fp32 passes share; N == 1: the per-sample rows ARE the parameter gradients
                GnBwdParams p{}; p.ca = g.ca; p.cb = g.cb; p.gamma = (const float*)rp(bs, g.gamma); p.groups = g.groups; p.DHW = g.DHW; p.N = g.N;
                p.nslab = g.nslab; p.partial = (float*)rp(bs, g.partial); p.gsum = gsum;
                p.dgamma_n = g.N == 1 ? dgamma : (float*)rp(bs, g.dgamma_n); p.dbeta_n = g.N == 1 ? dbeta : (float*)rp(bs, g.dbeta_n);
                if (g.fp32) {                // stats and apply on fp32 tensors, the fold kernel (p) is type agnostic
                    Gnb32Params q{}; q.dy = (const float*)rp(bs, g.dy); q.xa = (const float*)rp(bs, g.xa); q.xb = (const float*)rp(bs, g.xb);
                    q.ca = g.ca; q.cb = g.cb; q.ab = (const float*)rp(bs, g.ab); q.mr = (const float*)rp(bs, g.mr); q.gamma = p.gamma;
                    q.groups = g.groups; q.DHW = g.DHW; q.N = g.N; q.silu = g.silu; q.nslab = g.nslab; q.rows_per_slab = g.rows_per_slab;
                    q.partial = p.partial; q.gsum = gsum;
                    q.acc_a = (const float*)rp(bs, g.acc_a); q.acc_b = (const float*)rp(bs, g.acc_b); q.dxa = (float*)rp(bs, g.dxa); q.dxb = (float*)rp(bs, g.dxb);
                    launch_gnb32(q, p, dgamma, dbeta, s);
                    break;
                }
                p.dy = (const bf16_t*)rp(bs, g.dy); p.xa = (const bf16_t*)rp(bs, g.xa); p.xb = (const bf16_t*)rp(bs, g.xb);
                p.ab = (const float*)rp(bs, g.ab); p.mr = (const float*)rp(bs, g.mr); p.silu = g.silu; p.rows_per_slab = g.rows_per_slab;
                p.acc_a = (const bf16_t*)rp(bs, g.acc_a); p.acc_b = (const bf16_t*)rp(bs, g.acc_b);
                p.dxa = (bf16_t*)rp(bs, g.dxa); p.dxb = (bf16_t*)rp(bs, g.dxb);
                p.rows_per_block = g.rows_per_block; p.cs = (float*)rp(bs, g.cs);   // passes 2 + 3 in one launch where chunks > 0 (Builder::backward_gn decided)
                launch_gnb(p, g.chunks, dgamma, dbeta, s);
                break; }
            case OP_ATTN_BWD: {
                if (o.at.fp32) { const Attn32BwdParams q = attn_bwd_params<Attn32BwdParams>(o.at, bs); HIP_TRY(launch_attn32_bwd(q, s)); break; }
                const AttnBwdParams p = attn_bwd_params<AttnBwdParams>(o.at, bs);
                HIP_TRY(launch_attn_bwd(p, s));
                break; }
            case OP_ADD: {
                const ElemRec& e = o.el;
                if (e.fp32) { hipLaunchKernelGGL(add_f32_kernel, dim3(grid_for(e.n, 256, 4096)), dim3(256), 0, s, (const float*)rp(bs, e.a),
                                                 (const float*)rp(bs, e.b), (float*)rp(bs, e.out), (long)e.n); break; }
                launch_add_bf16((const bf16_t*)rp(bs, e.a), (const bf16_t*)rp(bs, e.b), (bf16_t*)rp(bs, e.out), (long)e.n, s);
                break; }
            case OP_SUMPOOL: {
                const ElemRec& e = o.el;
                if (e.fp32) { hipLaunchKernelGGL(sumpool2_f32_kernel, dim3(grid_for((long)e.N * e.D * e.H * e.W * (e.C / 4), 256, 4096)), dim3(256), 0, s,
                                                 (const float*)rp(bs, e.a), (float*)rp(bs, e.out), e.N, e.D, e.H, e.W, e.C); break; }
                launch_sumpool2((const bf16_t*)rp(bs, e.a), (bf16_t*)rp(bs, e.out), e.N, e.D, e.H, e.W, e.C, s);
                break; }
            case OP_LIN_DX: {
                const LinRec& l = o.lin;
                if (l.fp32) {               // fp32 weights
                    const float* w = (const float*)rp(bs, l.w);
                    if (!w) return fail(LDM_ERR_NOT_LOADED, "fp32 precision: the fp32 weight arena is empty");
                    hipLaunchKernelGGL(linear_bwd_dx_part_f32w_kernel, dim3((l.I + 255) / 256, l.B, l.nz), dim3(256), 0, s, w,
                                       (const float*)rp(bs, l.dy), (float*)rp(bs, l.part), l.I, l.O, l.dy_stride, l.B);
                    hipLaunchKernelGGL(linear_bwd_dx_fold_f32_kernel, dim3((l.I + 255) / 256, l.B), dim3(256), 0, s, (const float*)rp(bs, l.part),
                                       (const float*)rp(bs, l.x_pre), (float*)rp(bs, l.dx), l.I, l.nz, l.x_stride, l.B, l.silu);
                    break;
                }
                launch_lin_dx((const bf16_t*)rp(bs, l.w), (const float*)rp(bs, l.dy), (const float*)rp(bs, l.x_pre), (float*)rp(bs, l.dx),
                              (float*)rp(bs, l.part), l.B, l.I, l.O, l.dy_stride, l.x_stride, l.silu, l.nz, s);
                break; }
            case OP_VAE_HEADS_BWD: {
                const ElemRec& e = o.el;
                const float* ml = (const float*)rp(bs, e.ml); const float* z = (const float*)rp(bs, e.z);
                const float* g_mu = (const float*)rp(bs, e.g_mu); const float* g_sigma = (const float*)rp(bs, e.g_sigma);
                if (e.fp32) launch_vae_heads_bwd<float>((const float*)rp(bs, e.dz), e.c_dz, ml, z, g_mu, g_sigma, (float*)rp(bs, e.dy), e.N, e.L, e.C, e.DHW, s);
                else launch_vae_heads_bwd<bf16_t>((const bf16_t*)rp(bs, e.dz), e.c_dz, ml, z, g_mu, g_sigma, (bf16_t*)rp(bs, e.dy), e.N, e.L, e.C, e.DHW, s);
                break; }
            case OP_LIN_DW: {
                const LinRec& l = o.lin;
                if (l.fp32) { hipLaunchKernelGGL(linear_bwd_dw_f32_kernel, dim3(grid_for((long)l.O * l.I, 256, 1 << 24)), dim3(256), 0, s,
                                                 (const float*)rp(bs, l.dy), (const float*)rp(bs, l.x_pre), (float*)rp(bs, l.dW), (float*)rp(bs, l.db),
                                                 l.B, l.I, l.O, l.dy_stride, l.x_stride, l.silu); break; }
                launch_lin_dw((const float*)rp(bs, l.dy), (const float*)rp(bs, l.x_pre), (float*)rp(bs, l.dW), (float*)rp(bs, l.db),
                              l.B, l.I, l.O, l.dy_stride, l.x_stride, l.silu, s);
                break; }
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ================================================================================================ C ABI
extern "C" {

int ldm_version(void) { return LDM_ABI_VERSION; }
const char* ldm_last_error(void) { return g_err; }

int ldm_unet_create(const ldm_unet_cfg* cfg, ldm_model** out) {
    if (!cfg || !out) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (cfg->spatial_dims != 3) return fail(LDM_ERR_UNSUPPORTED, "only spatial_dims == 3 is implemented");
    if (cfg->num_levels < 1 || cfg->num_levels > LDM_MAX_LEVELS) return fail(LDM_ERR_BAD_ARG, "num_levels out of range");
    if (cfg->in_channels < 1 || cfg->out_channels < 1 || cfg->norm_num_groups < 1) return fail(LDM_ERR_BAD_ARG, "bad channel counts");
    for (int i = 0; i < cfg->num_levels; ++i) {
        if (cfg->num_res_blocks[i] < 1) return fail(LDM_ERR_BAD_ARG, "num_res_blocks[%d] < 1", i);
        const int hc = cfg->num_head_channels[i];
        const bool used = cfg->attention_levels[i] || i == cfg->num_levels - 1;          // the middle block always attends (MONAI)
        if (used && ((hc != 32 && hc != 64 && hc != 128 && hc != 256) || cfg->channels[i] % hc))
            return fail(LDM_ERR_UNSUPPORTED, "attention level %d: num_head_channels must be 32, 64, 128 or 256 and divide the level's "
                        "%d channels (got %d)", i, cfg->channels[i], hc);
    }
    std::unique_ptr<ldm_model> m(new ldm_model());
    m->type = 0; m->ucfg = *cfg;
    LDM_TRY(unet_register(m.get()));
    *out = m.release();
    return 0;
}

int ldm_vae_create(const ldm_vae_cfg* cfg, ldm_model** out) {
    if (!cfg || !out) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (cfg->spatial_dims != 3) return fail(LDM_ERR_UNSUPPORTED, "only spatial_dims == 3 is implemented");
    if (cfg->num_levels < 1 || cfg->num_levels > LDM_MAX_LEVELS) return fail(LDM_ERR_BAD_ARG, "num_levels out of range");
    if (cfg->in_channels < 1 || cfg->out_channels < 1 || cfg->latent_channels < 1 || cfg->latent_channels > 16)
        return fail(LDM_ERR_BAD_ARG, "bad channel counts");
    std::unique_ptr<ldm_model> m(new ldm_model());
    m->type = 1; m->vcfg = *cfg;
    LDM_TRY(vae_register(m.get()));
    *out = m.release();
    return 0;
}

void ldm_model_destroy(ldm_model* m) {
    if (!m) return;
    for (auto& g : m->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
    if (m->gsync.stream) (void)hipStreamDestroy(m->gsync.stream);
    if (m->gsync.stage) (void)hipFree(m->gsync.stage);
    for (auto e : m->gsync.ev) (void)hipEventDestroy(e);
    if (m->arena) (void)hipFree(m->arena);
    if (m->arena32) (void)hipFree(m->arena32);
    if (m->temb_tab) (void)hipFree(m->temb_tab);
    delete m;
}

int ldm_model_num_params(const ldm_model* m) { return m ? (int)m->params.size() : 0; }
const char* ldm_model_param_name(const ldm_model* m, int i) {
    return (m && i >= 0 && i < (int)m->params.size()) ? m->params[i].name.c_str() : nullptr;
}
int ldm_model_param_ndim(const ldm_model* m, int i) {
    return (m && i >= 0 && i < (int)m->params.size()) ? (int)m->params[i].shape.size() : -1;
}
const int64_t* ldm_model_param_shape(const ldm_model* m, int i) {
    return (m && i >= 0 && i < (int)m->params.size()) ? m->params[i].shape.data() : nullptr;
}
int64_t ldm_model_param_numel_total(const ldm_model* m) {
    int64_t t = 0; if (!m) return 0;
    for (auto& p : m->params) { int64_t n = 1; for (auto s : p.shape) n *= s; t += n; }
    return t;
}

static int ensure_arena(ldm_model* m) {
    if (m->arena) return 0;
    HIP_TRY(hipMalloc((void**)&m->arena, m->arena_bytes));
    HIP_TRY(hipMemset(m->arena, 0, m->arena_bytes));
    // the memset runs on the null stream and may still be in flight when this returns; the uploads that follow go to the
    // caller's stream, which need not synchronise with the null stream (non-blocking streams): wait here, once per model
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

static int ensure_arena32(ldm_model* m) {
    if (m->arena32) return 0;
    HIP_TRY(hipMalloc((void**)&m->arena32, 2 * m->arena_bytes + m->x3_bytes));
    HIP_TRY(hipMemset(m->arena32, 0, 2 * m->arena_bytes + m->x3_bytes));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}
// device-side re-pack of one parameter (fp32 MONAI layout) into the fp32 arena
static void pack32_device(ldm_model* m, const ParamDesc& d, const float* src, hipStream_t s) {
    if (d.kind == PK_VEC_F32) return;
    float* dst = (float*)(m->arena32 + 2 * d.dst_off);
    const bool lin = d.kind == PK_LINEAR_W;
    const int taps = lin ? 1 : d.k * d.k * d.k, cin_s = lin ? d.cin : d.cin_s, cout_pad = lin ? d.cout : d.cout_pad, row_off = lin ? 0 : d.row_off;
    const long total = (long)taps * d.cout * cin_s;
    hipLaunchKernelGGL(param_pack_f32_kernel, dim3(grid_for(total, 256, 8192)), dim3(256), 0, s, src, dst, taps, d.cout, d.cin, cin_s, cout_pad, row_off);
}

int ldm_model_load_param(ldm_model* m, const char* name, const float* src, size_t numel) {
    if (!m || !name || !src) return fail(LDM_ERR_BAD_ARG, "null argument");
    auto it = m->pindex.find(name);
    if (it == m->pindex.end()) return fail(LDM_ERR_BAD_ARG, "unknown parameter '%s'", name);
    ParamDesc& d = m->params[it->second];
    size_t expect = 1; for (auto s : d.shape) expect *= (size_t)s;
    if (expect != numel) return fail(LDM_ERR_BAD_ARG, "parameter '%s': expected %zu elements, got %zu", name, expect, numel);
    LDM_TRY(ensure_arena(m));
    if (d.kind == PK_VEC_F32) {
        HIP_TRY(hipMemcpy(m->arena + d.dst_off, src, numel * 4, hipMemcpyHostToDevice));
    } else if (d.kind == PK_LINEAR_W) {
        std::vector<uint16_t> tmp(numel);
        for (size_t k = 0; k < numel; ++k) tmp[k] = host_f2bf(src[k]);
        HIP_TRY(hipMemcpy(m->arena + d.dst_off, tmp.data(), numel * 2, hipMemcpyHostToDevice));
    } else {   // PK_CONV_W: [cout][cin][kd][kh][kw] fp32 -> [tap][cout_pad][cin_s] bf16 rows row_off..row_off+cout
        const int taps = d.k * d.k * d.k;
        std::vector<uint16_t> tmp((size_t)d.cout * d.cin_s);
        for (int t = 0; t < taps; ++t) {
            std::fill(tmp.begin(), tmp.end(), (uint16_t)0);
            for (int co = 0; co < d.cout; ++co)
                for (int ci = 0; ci < d.cin; ++ci)
                    tmp[(size_t)co * d.cin_s + ci] = host_f2bf(src[((size_t)co * d.cin + ci) * taps + t]);
            char* dst = m->arena + d.dst_off + ((size_t)t * d.cout_pad + d.row_off) * d.cin_s * 2;
            HIP_TRY(hipMemcpy(dst, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
        }
    }
    if (m->precision == 1 && d.kind != PK_VEC_F32) {     // the unrounded copy for the fp32 precision mode
        LDM_TRY(ensure_arena32(m));
        if (d.kind == PK_LINEAR_W) {
            HIP_TRY(hipMemcpy(m->arena32 + 2 * d.dst_off, src, numel * 4, hipMemcpyHostToDevice));
        } else {
            const int taps = d.k * d.k * d.k;
            std::vector<float> tmp((size_t)d.cout * d.cin_s);
            for (int t = 0; t < taps; ++t) {
                std::fill(tmp.begin(), tmp.end(), 0.f);
                for (int co = 0; co < d.cout; ++co)
                    for (int ci = 0; ci < d.cin; ++ci)
                        tmp[(size_t)co * d.cin_s + ci] = src[((size_t)co * d.cin + ci) * taps + t];
                char* dst = m->arena32 + 2 * (d.dst_off + ((size_t)t * d.cout_pad + d.row_off) * d.cin_s * 2);
                HIP_TRY(hipMemcpy(dst, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
            }
        }
    }
    if (!d.loaded) { d.loaded = true; m->loaded_count++; }
    m->derived_dirty = true; m->temb_tab_valid = false;
    return 0;
}

// phase weights of the upsample convs, rebuilt (stream-ordered) after a parameter upload: called by the inference entries
static int ensure_derived(ldm_model* m, hipStream_t s) {
    if (!m->derived_dirty) return 0;
    for (const auto& iw : m->im2col_ws)
        launch_im2col_weights((const bf16_t*)(m->arena + iw.w_off), (bf16_t*)(m->arena + iw.wi_off), iw.cout_pad, iw.cin_s, iw.cin, iw.Kp, s);
    for (const auto& pw : m->phase_ws)
        launch_phase_weights((const bf16_t*)(m->arena + pw.w_off), (bf16_t*)(m->arena + pw.wp_off), pw.cout_pad, pw.cin_s, s);
    if (m->precision == 1 && m->arena32)
        for (const auto& xw : m->x3p_ws)
            launch_x3_phase_weights((const float*)(m->arena32 + 2 * xw.w_off), (bf16_t*)(m->arena32 + 2 * m->arena_bytes + xw.x3p_off), xw.cout_pad, xw.cin_s, s);
    if (m->precision == 1 && m->arena32)
        for (const auto& xw : m->x3_ws)
            launch_x3_weights((const float*)(m->arena32 + 2 * xw.w_off), (bf16_t*)(m->arena32 + 2 * m->arena_bytes + xw.x3_off), xw.rows, xw.cin_s, s);
    HIP_TRY(hipGetLastError());
    m->derived_dirty = false;
    return 0;
}

static int get_plan(ldm_model* m, const char* kind, int B, int D, int H, int W, std::shared_ptr<Plan>* out, int tap_mode = 0) {
    if (B < 1 || D < 1 || H < 1 || W < 1 || D > 255 * 8 || H > 255 * 8 || W > 255 * 8) return fail(LDM_ERR_BAD_ARG, "bad shape");
    const bool train = kind[0] == 't';
    const bool hp = m->precision == 1;
    // backward variants of the UNet's training plan (same forward ops and activation offsets): "train" parameter gradients, "train_px"
    // parameter and input gradients, "train_x" input gradients only (the data-only backward)
    const int bwd_mode = !strcmp(kind, "train_px") ? 3 : !strcmp(kind, "train_x") ? 2 : 1;
    char key[96]; snprintf(key, sizeof key, "%s:%d:%d:%d:%d:p%d:t%d", kind, B, D, H, W, hp ? 1 : 0, tap_mode);
    auto it = m->plans.find(key);
    if (it != m->plans.end()) { *out = it->second; return 0; }
    std::shared_ptr<Plan> p(new Plan());
    if (m->type == 0) LDM_TRY(unet_build(m, B, D, H, W, p.get(), train, hp, tap_mode, strcmp(kind, "unet_tab") == 0 || strcmp(kind, "unet_cfg_tab") == 0,
                                     strncmp(kind, "unet_cfg", 8) == 0, bwd_mode));
    else if (train) LDM_TRY(vae_build_train(m, B, D, H, W, p.get(), hp));
    else if (kind[0] == 'e') LDM_TRY(vae_build_encode(m, B, D, H, W, p.get(), hp, tap_mode));
    else if (!strcmp(kind, "dec_x")) LDM_TRY(vae_build_decode_grad(m, B, D, H, W, p.get(), hp));
    else LDM_TRY(vae_build_decode(m, B, D, H, W, p.get(), hp, tap_mode));
    m->plans[key] = p; *out = p;
    return 0;
}

static int check_ready(ldm_model* m, const void* ws, size_t ws_bytes, const Plan& p) {
    if (m->loaded_count != (int)m->params.size()) {
        for (auto& d : m->params) if (!d.loaded)
            return fail(LDM_ERR_NOT_LOADED, "parameter '%s' (and %d others) not uploaded", d.name.c_str(),
                        (int)m->params.size() - m->loaded_count - 1);
    }
    if (!ws || ws_bytes < p.ws_bytes) return fail(LDM_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", p.ws_bytes, ws_bytes);
    if (((uintptr_t)ws) & 255) return fail(LDM_ERR_BAD_ARG, "workspace must be 256-byte aligned");
    if (p.wt_tab.ready() || p.exp_tab.ready() || p.cs_tab.ready()) return fail(LDM_ERR_HIP, "descriptor table upload failed");
    return 0;
}

// the plan of (kind, shape), refused unless the model and the caller's workspace are ready to run it
static int ready_plan(ldm_model* m, const char* kind, int B, int D, int H, int W, const void* ws, size_t ws_bytes, std::shared_ptr<Plan>* out,
                      int tap_mode = 0) {
    LDM_TRY(get_plan(m, kind, B, D, H, W, out, tap_mode));
    return check_ready(m, ws, ws_bytes, **out);
}
// the bases every plan run starts from: the workspace and the two weight arenas; the caller adds its tensors
static Bases model_bases(const ldm_model* m, void* workspace) {
    Bases bs{}; bs.p[BASE_WS] = (char*)workspace; bs.p[BASE_W] = m->arena; bs.p[BASE_W32] = m->arena32;
    return bs;
}

size_t ldm_unet_workspace_bytes(ldm_model* m, int B, int D, int H, int W) {
    if (!m || m->type != 0) { fail(LDM_ERR_BAD_ARG, "not a UNet handle"); return 0; }
    std::shared_ptr<Plan> p; if (get_plan(m, "unet", B, D, H, W, &p)) return 0;
    return p->ws_bytes;
}

// ---- device-resident sampler (fused scheduler step with in-kernel Philox noise) ----------------------------------------------
static std::atomic<uint64_t> g_sampler_uid{0};
struct ldm_sampler;
// ldm_likelihood_*: `rows` is the device row table, step counter and timesteps of the schedule, held as a sampler (never stepped as one)
// so that the reset kernel, the time-embedding table and the graph cache's identity rules serve it; `host` mirrors the rows for the
// entries that pass one by value, `next` counts the steps taken since the last reset, `noise` is what the last reset was given.
struct ldm_likelihood {
    ldm_sampler* rows = nullptr; std::vector<float> host; int n_steps = 0, pred = 0, clip = 1, next = 0;
    unsigned seed_lo = 0, seed_hi = 0; float half_bin = 0.f; const float* noise = nullptr;
};
struct ldm_sampler {
    float* coef = nullptr; SamplerState* st = nullptr; int n_steps = 0, kind = 0, clip = 1, pred = PRED_EPSILON; unsigned seed_lo = 0, seed_hi = 0;
    uint64_t uid = ++g_sampler_uid;                  // never reused (graph-replay cache key)
    // kind SAMPLER_PNDM: coef rows are PNDM_ROW floats (norm_elem.h) and the step needs the caller-owned multistep state bound by
    // ldm_sampler_bind_state: 6 regions of state_n floats.  kind SAMPLER_DPM (DPM-Solver++): DPM_ROW floats per row, and the state is
    // one region of state_n floats, the previous call's x0_hat
    float* state = nullptr; int64_t state_n = 0;
    std::vector<float> ts;                           // host copy of the schedule's timesteps in sampling order (key of the model's time-embedding table)
    // repaint (ldm_sampler_create_repaint): coef rows are REPAINT_ROW floats (repaint.h) on the base `kind` (DDPM, DDIM or flow) and the
    // step needs the caller-owned known latent and keep mask bound by ldm_sampler_bind_known (which renews `uid`)
    int repaint = 0, known_batch = 0; const float* known = nullptr; const float* keep = nullptr; int64_t rp_per_sample = 0, rp_dhw = 0;
};
enum { SAMPLER_DDPM = 0, SAMPLER_DDIM = 1, SAMPLER_PNDM = 2, SAMPLER_RFLOW = 3, SAMPLER_DPM = 4 };
static bool sampler_multistep(const ldm_sampler* sp) { return sp->kind == SAMPLER_PNDM || sp->kind == SAMPLER_DPM; }
static const char* sampler_multistep_name(const ldm_sampler* sp) { return sp->kind == SAMPLER_DPM ? "DPM-Solver++" : "PNDM"; }
// floats per row of the sampler's table; t sits in slot 5 of every layout
static int sampler_row_len(const ldm_sampler* sp) {
    return sp->repaint ? (int)REPAINT_ROW : sp->kind == SAMPLER_PNDM ? (int)PNDM_ROW : sp->kind == SAMPLER_DPM ? (int)DPM_ROW : 8;
}
// repaint: a step of n elements on `samples` samples needs a binding of that shape; checked before anything is launched
static int repaint_check(const ldm_sampler* sp, int64_t n, int64_t samples) {
    if (!sp->repaint) return 0;
    if (!sp->known || !sp->keep) return fail(LDM_ERR_BAD_ARG, "repaint sampler without a known latent and keep mask: call ldm_sampler_bind_known first");
    if (samples < 1 || n != samples * sp->rp_per_sample)
        return fail(LDM_ERR_BAD_ARG, "repaint sampler: bound for samples of %lld elements, the step has %lld elements on %lld samples",
                    (long long)sp->rp_per_sample, (long long)n, (long long)samples);
    if (sp->known_batch != 1 && sp->known_batch != samples)
        return fail(LDM_ERR_BAD_ARG, "repaint sampler: known_batch must be 1 or the step's %lld samples, got %d", (long long)samples, sp->known_batch);
    return 0;
}
static int repaint_launch(ldm_sampler* sp, const float* m, float* x, float* x0_out, int64_t n, float* tbuf, int B, hipStream_t s,
                          const WinGeom* geom, float* xw, int C);
// the device step of a DPM-Solver++ sampler (defined with its entries at the end of the file, where its kernels are instantiated: the
// code object keeps the layout of every kernel that was there before them)
static int dpm_launch(ldm_sampler* sp, const float* m, float* x, float* x0_out, int64_t n, float* tbuf, int B, hipStream_t s,
                      const WinGeom* geom, float* xw, int C);
// a window grid over one full latent (sliding-window sampling, window.h; built and checked by ldm_window_grid_create below)
static std::atomic<uint64_t> g_grid_uid{0};
struct ldm_window_grid {
    int dims[3] = {0, 0, 0}, roi[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    char* dev = nullptr;                             // starts | weight tables | cover tables, per axis
    WinGeom geom{};
    uint64_t uid = ++g_grid_uid;                     // never reused (graph-replay cache key)
    int64_t n_windows() const { return (int64_t)n[0] * n[1] * n[2]; }
    int64_t roi_vox() const { return (int64_t)roi[0] * roi[1] * roi[2]; }
    int64_t vox() const { return (int64_t)dims[0] * dims[1] * dims[2]; }
};
// The prediction type picks a kernel instantiation (no per-element branch on it): launch(P) is called with P() == pred as a constant
// expression.  The caller has checked pred; SAMPLE = false: the PNDM kernels, which exist for epsilon and v_prediction only.
extern "C++" template <bool SAMPLE = true, class Launch>
static void with_pred(int pred, Launch&& launch) {
    if constexpr (SAMPLE) if (pred == PRED_SAMPLE) return launch(std::integral_constant<int, PRED_SAMPLE>{});
    if (pred == PRED_V) return launch(std::integral_constant<int, PRED_V>{});
    launch(std::integral_constant<int, PRED_EPSILON>{});
}
// PNDM / DPM-Solver++: the step of an n-element latent needs a bound state buffer for exactly n elements; checked before anything is launched
static int sampler_check_state(const ldm_sampler* sp, int64_t n) {
    if (!sampler_multistep(sp)) return 0;
    if (!sp->state) return fail(LDM_ERR_BAD_ARG, "%s sampler without a state buffer: call ldm_sampler_bind_state first", sampler_multistep_name(sp));
    if (sp->state_n != n) return fail(LDM_ERR_BAD_ARG, "%s sampler: the state buffer is bound for %lld elements, the step has %lld",
                                      sampler_multistep_name(sp), (long long)sp->state_n, (long long)n);
    return 0;
}
// what a device step takes from the sampler: table, counter, rule, seed and multistep state; the caller adds the tensors
static StepParams step_params(const ldm_sampler* sp) {
    StepParams p{}; p.coef = sp->coef; p.st = sp->st; p.n_steps = sp->n_steps; p.kind = sp->kind; p.clip = sp->clip;
    p.seed_lo = sp->seed_lo; p.seed_hi = sp->seed_hi; p.state = sp->state;
    return p;
}
// The sampler's kind and prediction type pick a step rule (norm_elem.h StepRule): launch(P, F) is called with the prediction type P()
// and the family F() as constant expressions.  PNDM exists for epsilon and v_prediction, the flow rule once.  DDPM / DDIM stands first
// because the kernels are emitted in this order, and theirs are the ones on the headline path.
extern "C++" template <class Launch>
static void with_rule(const ldm_sampler* sp, Launch&& launch) {
    if (sp->kind <= SAMPLER_DDIM) return with_pred(sp->pred, [&](auto P) { launch(P, std::integral_constant<int, STEP_DDPM>{}); });
    if (sp->kind == SAMPLER_PNDM) return with_pred<false>(sp->pred, [&](auto P) { launch(P, std::integral_constant<int, STEP_PNDM>{}); });
    launch(std::integral_constant<int, PRED_EPSILON>{}, std::integral_constant<int, STEP_FLOW>{});
}
// One device step on the n elements of x: m is the model output on the full latent or, with a window geometry, on the windows
// [nW][C][roi] of x [C][dims], blended inside the kernel, and the new x goes back into the windows xw as well.
static int sampler_launch(ldm_sampler* sp, const float* m, float* x, float* x0_out, int64_t n, float* tbuf, int B, hipStream_t s,
                          const WinGeom* geom = nullptr, float* xw = nullptr, int C = 0) {
    if (sp->kind == SAMPLER_PNDM && x0_out) return fail(LDM_ERR_BAD_ARG, "PNDM has no x0_hat: x0_out must be NULL");
    LDM_TRY(sampler_check_state(sp, n));
    if (sp->repaint) return repaint_launch(sp, m, x, x0_out, n, tbuf, B, s, geom, xw, C);
    if (sp->kind == SAMPLER_DPM) return dpm_launch(sp, m, x, x0_out, n, tbuf, B, s, geom, xw, C);
    StepParams p = step_params(sp); p.m = m; p.x = x; p.x0_out = x0_out; p.n = (long)n; p.tbuf = tbuf; p.B = B; p.xw = xw; p.C = C;
    const dim3 grid(grid_for((n + 3) / 4, 256, 1024));
    with_rule(sp, [&](auto P, auto F) {
        if (!geom) hipLaunchKernelGGL((sampler_step_kernel<P(), F()>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((window_blend_step_kernel<P(), F()>), grid, dim3(256), 0, s, *geom, p);
    });
    return 0;
}

// The stacked time_emb_proj outputs for every step of `sp`'s schedule, [n_steps][tproj_rows] fp32, built by the forward plan's own
// kernels (sinusoid -> Linear -> SiLU -> Linear -> SiLU -> stacked projections) at batch n_steps, so row k is bit-identical to what
// the plan computes for t = ts[k].  Rebuilt after a parameter upload / optimizer step, a precision switch or for another schedule;
// a table that moves in memory invalidates the model's cached graphs (they hold its address).  LDM_TEMB_TABLE=0: never used.
static bool temb_table_enabled() { static const int v = ldm_knob("LDM_TEMB_TABLE", 1); return v != 0; }
static int ensure_temb_table(ldm_model* m, const ldm_sampler* sp, hipStream_t s) {
    if (m->temb_tab_valid && m->temb_tab_prec == m->precision && m->temb_tab_ts == sp->ts) return 0;
    const int n = sp->n_steps, rows = m->tproj_rows, c0 = m->ucfg.channels[0], temb = 4 * c0;
    const bool hp = m->precision == 1;
    if (hp && !m->arena32) return fail(LDM_ERR_NOT_LOADED, "fp32 precision: the fp32 weight arena is empty");
    const size_t need = (size_t)n * rows * 4;
    if (need > m->temb_tab_cap) {
        HIP_TRY(hipDeviceSynchronize());                                   // a replaying graph may still read the old table
        for (auto& g : m->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
        m->graphs.clear();
        if (m->temb_tab) (void)hipFree(m->temb_tab);
        m->temb_tab = nullptr; m->temb_tab_cap = 0;
        HIP_TRY(hipMalloc((void**)&m->temb_tab, need));
        m->temb_tab_cap = need;
    }
    float* tmp = nullptr;                                                  // t [n] | sinusoid [n][c0] | e1 [n][temb] | e2 [n][temb]
    HIP_TRY(hipMalloc((void**)&tmp, (size_t)n * (1 + c0 + 2 * temb) * 4));
    float* d_t = tmp; float* d_sin = tmp + n; float* d_e1 = d_sin + (size_t)n * c0; float* d_e2 = d_e1 + (size_t)n * temb;
    hipError_t e = hipMemcpyAsync(d_t, sp->ts.data(), (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        const LinW& l0 = m->lins.at("time_embed.0"); const LinW& l2 = m->lins.at("time_embed.2");
        launch_sinusoid((const float*)d_t, d_sin, n, c0, s);
        auto gemv = [&](size_t w_off, size_t b_off, const float* xin, float* y, int I, int O, int silu) {
            launch_gemv(hp ? m->arena32 + 2 * w_off : m->arena + w_off, hp, (const float*)(m->arena + b_off), xin, y, n, I, O, I, O, silu, s);
        };
        gemv(l0.w_off, l0.b_off, d_sin, d_e1, c0, temb, 0);
        gemv(l2.w_off, l2.b_off, d_e1, d_e2, temb, temb, 1);
        gemv(m->tproj_w_off, m->tproj_b_off, d_e2, m->temb_tab, temb, rows, 1);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);                  // the temporaries go away below; one-off per upload
    }
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(LDM_ERR_HIP, "time-embedding table: %s", hipGetErrorString(e));
    m->temb_tab_ts = sp->ts; m->temb_tab_prec = m->precision; m->temb_tab_valid = true;
    return 0;
}

// Graph replay of one call's launch sequence `run_all`: recorded once per key, replayed as ONE hipGraphLaunch afterwards.  The first
// sight of a key runs eagerly.
extern "C++" template <class RunAll>
static int graph_run(ldm_model* m, const ldm_model::GraphKey& key, hipStream_t stream, RunAll&& run_all) {
    ldm_model::GraphEntry* ge = nullptr;
    for (size_t k = 0; k < m->graphs.size();) {          // entries recorded for a sampler / grid that has since been destroyed at this address
        const auto& g = m->graphs[k].key;
        if ((key.ptr[6] && g.ptr[6] == key.ptr[6] && g.sampler_uid != key.sampler_uid) ||
            (key.grid && g.grid == key.grid && g.grid_uid != key.grid_uid)) {
            if (m->graphs[k].exec) (void)hipGraphExecDestroy(m->graphs[k].exec);
            m->graphs.erase(m->graphs.begin() + k);
        } else ++k;
    }
    for (auto& g : m->graphs) if (!memcmp(&g.key, &key, sizeof key)) { ge = &g; break; }
    if (!ge) {
        if (m->graphs.size() >= 16) {                    // bounded cache: drop the oldest entry
            if (m->graphs.front().exec) (void)hipGraphExecDestroy(m->graphs.front().exec);
            m->graphs.erase(m->graphs.begin());
        }
        m->graphs.emplace_back(); ge = &m->graphs.back();
        memcpy(&ge->key, &key, sizeof key); ge->seen = 0; ge->exec = nullptr;   // memcpy: the padding travels too
    }
    if (ge->exec) { HIP_TRY(hipGraphLaunch(ge->exec, stream)); return 0; }
    if (ge->seen++ == 0) return run_all(stream);         // first sight: eager (also warms one-time set-up)
    hipGraph_t graph = nullptr;
    if (!m->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = run_all(m->cap_stream);
    const hipError_t ec = hipStreamEndCapture(m->cap_stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ec != hipSuccess || !graph) return fail(LDM_ERR_HIP, "stream capture failed: %s", hipGetErrorString(ec));
    HIP_TRY(hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    HIP_TRY(hipGraphLaunch(ge->exec, stream));
    return 0;
}

struct Guide { float w, fill; };                         // classifier-free guidance of one step: scale and the unconditional half's condition value
// The tail of a likelihood step (ldm_unet_likelihood_step): the term and finalize kernels on the row the device counter points at.
// `sp` of the forward is then the handle's row table and counter (the time-embedding table is keyed by its timesteps).
struct LikStep { const ldm_likelihood* lk; const float* x0; float* kl_map; float* terms; float* total; void* scratch; };
static int likelihood_tail(const LikStep& ls, float* x_t, const float* m_out, float* tbuf, int B, int64_t per_sample, hipStream_t s);
// One UNet step, as every entry below describes it: the forward plan on `total` samples of D x H x W in chunks of B, then a tail.
// x [total][x_channels][DHW], cond [total][cond_channels][DHW] or null, out [total][out_channels][DHW].  The full-latent entries run one
// chunk of B = total samples and no grid; a windowed step runs the windows xw (= x here) of `grid` in ceil(total / B) chunks, the last
// one ragged.  guide: every chunk runs the guided plan at 2 B and is combined into out: in place on the doubled out of the full latent,
// from the pair buffer behind the workspace for windows.  Tail: none without a sampler (a plain forward), the likelihood terms with
// `lik`, else the sampler's step on `latent` (x itself, or the full volume the windows blend into).  The entries fill the record in
// this order and leave out what they do not have.
struct StepArgs {
    const float* x; int x_channels; const float* cond; int cond_channels; float* tbuf; float* out;
    int B; int64_t total; int D, H, W;
    void* workspace; size_t workspace_bytes; void* stream;
    ldm_sampler* sp; float* latent; const Guide* guide; const LikStep* lik; const ldm_window_grid* grid;
};
static int unet_step(ldm_model* m, StepArgs a) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!a.x || !a.tbuf || !a.out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!a.cond) a.cond_channels = 0;
    const Guide* const guide = a.guide; ldm_sampler* const sp = a.sp; const ldm_window_grid* const grid = a.grid;
    const int gm = guide ? 2 : 1;                        // a guided chunk of B samples runs its plan at 2 B: (unconditional | conditional)
    // a denoising step driven by a sampler knows its timestep as a step INDEX on the device: the time-embedding chain becomes one row copy
    const bool tab = sp != nullptr && temb_table_enabled() && m->tproj_rows % 4 == 0;
    const char* kind = guide ? (tab ? "unet_cfg_tab" : "unet_cfg") : tab ? "unet_tab" : "unet";
    const int ragged = a.B > 0 ? (int)(a.total % a.B) : 0;   // B < 1 is refused with the plan
    std::shared_ptr<Plan> p, p2;
    LDM_TRY(ready_plan(m, kind, gm * a.B, a.D, a.H, a.W, a.workspace, a.workspace_bytes, &p));
    if (ragged) LDM_TRY(ready_plan(m, kind, gm * ragged, a.D, a.H, a.W, a.workspace, a.workspace_bytes, &p2));
    const int64_t per_out = (int64_t)m->ucfg.out_channels * a.D * a.H * a.W, per_x = (int64_t)a.x_channels * a.D * a.H * a.W;
    // guided windows: the doubled output of a chunk lands behind the plan's workspace (ldm_unet_guided_workspace_bytes counts it)
    float* pair = nullptr;
    if (guide && grid) {
        const size_t pair_off = rup_sz(std::max(p->ws_bytes, p2 ? p2->ws_bytes : (size_t)0), 256), need = pair_off + (size_t)2 * a.B * per_out * 4;
        if (a.workspace_bytes < need)
            return fail(LDM_ERR_WORKSPACE, "workspace too small for the guided windows: need %zu bytes, got %zu", need, a.workspace_bytes);
        pair = (float*)((char*)a.workspace + pair_off);
    }
    if (tab) LDM_TRY(ensure_temb_table(m, sp, (hipStream_t)a.stream));
    Bases bs = model_bases(m, a.workspace);
    bs.p[BASE_IO2] = (char*)a.tbuf;
    if (tab) { bs.p[BASE_TTAB] = (char*)m->temb_tab; bs.p[BASE_SST] = (char*)sp->st; bs.sampler_steps = sp->n_steps; }
    if (guide) bs.guide_fill = guide->fill;
    const int rt[2] = {a.x_channels, a.cond_channels};
    LDM_TRY(ensure_derived(m, (hipStream_t)a.stream));
    // one step = the forward plan chunk by chunk, then the tail on the same stream
    auto run_all = [&](hipStream_t s) -> int {
        for (int64_t b0 = 0; b0 < a.total; b0 += a.B) {
            const bool last = b0 + a.B > a.total;
            float* dst = a.out + b0 * per_out;
            float* raw = pair ? pair : dst;              // where the plan writes: the chunk's doubled output when guided
            Bases cb = bs;
            cb.p[BASE_IO0] = (char*)(a.x + b0 * per_x);
            cb.p[BASE_IO1] = a.cond ? (char*)(a.cond + b0 * a.cond_channels * a.D * a.H * a.W) : nullptr;
            cb.p[BASE_IO3] = (char*)raw;
            LDM_TRY(run_plan(last ? *p2 : *p, cb, rt, s));
            if (guide) {
                const int64_t ne = (last ? ragged : a.B) * per_out;
                guided_combine_launch(raw, raw + ne, guide->w, dst, ne, s);
            }
        }
        if (a.lik) return likelihood_tail(*a.lik, a.latent, a.out, a.tbuf, a.B, per_out, s);
        if (!sp) return 0;
        if (!grid) return sampler_launch(sp, a.out, a.latent, nullptr, a.total * per_out, a.tbuf, gm * a.B, s);
        return sampler_launch(sp, a.out, a.latent, nullptr, grid->vox() * a.x_channels, a.tbuf, gm * a.B, s, &grid->geom, const_cast<float*>(a.x), a.x_channels);
    };
    if (!m->graph_mode || g_prof.on || g_plan_trace.on) return run_all((hipStream_t)a.stream);
    // ---- graph replay: same launches, recorded once per key
    ldm_model::GraphKey key; memset(&key, 0, sizeof key);
    key.plan[0] = p.get(); key.plan[1] = p2.get();
    const void* ptr[8] = {a.x, a.cond, a.tbuf, a.out, a.workspace, a.stream, sp, a.latent};
    memcpy(key.ptr, ptr, sizeof ptr); key.rt[0] = rt[0]; key.rt[1] = rt[1]; key.chunk = a.B;
    if (sp) { key.sampler_uid = sp->uid; key.sampler_state = sp->state; }
    if (grid) { key.grid = grid; key.grid_uid = grid->uid; }
    if (guide) { key.guide[0] = guide->w; key.guide[1] = guide->fill; }
    if (a.lik) { const void* lp[6] = {a.lik->x0, a.lik->lk->noise, a.lik->kl_map, a.lik->terms, a.lik->total, a.lik->scratch}; memcpy(key.lik, lp, sizeof lp); }
    return graph_run(m, key, (hipStream_t)a.stream, run_all);
}
int ldm_unet_forward(ldm_model* m, const float* x, int x_channels, const float* cond, int cond_channels,
                     const float* timesteps, float* out, int B, int D, int H, int W,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return unet_step(m, {x, x_channels, cond, cond_channels, (float*)timesteps, out, B, B, D, H, W, workspace, workspace_bytes, stream});
}

/* The tail of both constructors: the table on the device, a zeroed step counter, and the host copy of the timesteps (slot 5 of each
 * `row_len`-float row).  The caller has checked the table and fills in kind / pred / clip / seed. */
static int sampler_alloc(const float* coef_host, int row_len, int n_steps, std::unique_ptr<ldm_sampler>* out) {
    std::unique_ptr<ldm_sampler> sp(new ldm_sampler());
    const size_t bytes = (size_t)n_steps * row_len * 4;
    HIP_TRY(hipMalloc((void**)&sp->coef, bytes));
    HIP_TRY(hipMemcpy(sp->coef, coef_host, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void**)&sp->st, 256));
    HIP_TRY(hipMemset(sp->st, 0, 256));
    HIP_TRY(hipDeviceSynchronize());
    sp->n_steps = n_steps;
    sp->ts.resize(n_steps); for (int k = 0; k < n_steps; ++k) sp->ts[k] = coef_host[(size_t)k * row_len + 5];
    *out = std::move(sp);
    return 0;
}
/* Sampler: coef_host = [n_steps][8] fp32 rows {1/sqrt(abar_t), sqrt(1 - abar_t), c0, c1 (DDPM: coefficient of x_t | DDIM: direction
 * coefficient of eps), sigma, t, sqrt(abar_t), 1/sqrt(1 - abar_t)} in sampling order (the host mirror computes them exactly as MONAI
 * does and as DDPMScheduler.step / DDIMScheduler.step pass them to ldm_scheduler_step); kind 0 = DDPM, 1 = DDIM; pred 0 epsilon, 1 sample,
 * 2 v_prediction.  Noise: Philox4x32-10(counter = (element quad, step), key = seed). */
int ldm_sampler_create(const float* coef_host, int n_steps, int kind, int pred, int clip, uint64_t seed, ldm_sampler** out) {
    if (!coef_host || n_steps < 1 || kind < 0 || kind > 1 || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    std::unique_ptr<ldm_sampler> sp; LDM_TRY(sampler_alloc(coef_host, 8, n_steps, &sp));
    sp->kind = kind; sp->pred = pred; sp->clip = clip ? 1 : 0; sp->seed_lo = (unsigned)seed; sp->seed_hi = (unsigned)(seed >> 32);
    *out = sp.release();
    return 0;
}
/* A PNDM sampler (PRK warm-up + PLMS): coef_host = [n_steps][LDM_PNDM_ROW] fp32 rows, one per UNet call in sampling order
 * (norm_elem.h: {cx, ce, sqrt(abar_t), sqrt(1 - abar_t), flags, t, wm, w1, w2, w3, wacc, am, head, 0, 0, 0}); pred 0 epsilon or 2
 * v_prediction.  The row program is replayed here once: a row that reads a history slot, the saved sample or the accumulator before an
 * earlier row wrote it is refused, which is why the state buffer never needs zeroing and ldm_sampler_reset (step counter := 0) rewinds
 * the whole multistep state.  No noise, no clipping. */
int ldm_sampler_create_pndm(const float* coef_host, int n_steps, int pred, ldm_sampler** out) {
    if (!coef_host || n_steps < 1 || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred != PRED_EPSILON && pred != PRED_V) return fail(LDM_ERR_BAD_ARG, "PNDM takes prediction type 0 (epsilon) or 2 (v_prediction), got %d", pred);
    static_assert(PNDM_ROW == LDM_PNDM_ROW, "row stride of the header");
    int pushes = 0; bool saved = false, acc = false;
    for (int k = 0; k < n_steps; ++k) {
        const float* r = coef_host + (size_t)k * PNDM_ROW;
        const PndmCoef c = pndm_coef(r);
        if (r[4] != (float)c.flags || c.flags < 0 || c.flags >= 32 || r[12] != (float)c.head || c.head != pushes)
            return fail(LDM_ERR_BAD_ARG, "PNDM row %d: bad flags / head (head must count the pushes of the rows before it)", k);
        if ((c.flags & PNDM_ACC_SET) && (c.flags & PNDM_ACC_ADD)) return fail(LDM_ERR_BAD_ARG, "PNDM row %d: accumulator both set and added to", k);
        const int depth = c.w3 != 0.f ? 3 : c.w2 != 0.f ? 2 : c.w1 != 0.f ? 1 : 0;
        if (depth > pushes) return fail(LDM_ERR_BAD_ARG, "PNDM row %d reads %d history slots, %d written so far", k, depth, pushes);
        if ((c.flags & PNDM_USE_SAVED) && !saved) return fail(LDM_ERR_BAD_ARG, "PNDM row %d reads the saved sample before any row saved one", k);
        if ((c.wacc != 0.f || (c.flags & PNDM_ACC_ADD)) && !acc) return fail(LDM_ERR_BAD_ARG, "PNDM row %d reads the accumulator before any row set it", k);
        if (c.flags & PNDM_PUSH) ++pushes;
        if (c.flags & PNDM_SAVE) saved = true;
        if (c.flags & PNDM_ACC_SET) acc = true;
    }
    std::unique_ptr<ldm_sampler> sp; LDM_TRY(sampler_alloc(coef_host, PNDM_ROW, n_steps, &sp));
    sp->kind = SAMPLER_PNDM; sp->pred = pred; sp->clip = 0;
    *out = sp.release();
    return 0;
}
/* A rectified-flow sampler (MONAI >= 1.4 RFlowScheduler.step over its timesteps, restated): coef_host = [n_steps][8] fp32 rows
 * {dt, tau, 0, 0, 0, t, 0, 0} in sampling order, dt = (t - t_next) / T and tau = t / T (schedulers.py computes them in fp64 and rounds
 * once); a step is x := x + dt m, x0_hat = x + tau m.  No noise, no clipping, no state: ldm_sampler_noise and ldm_sampler_bind_state
 * refuse such a sampler; every other ldm_sampler_* entry and the two denoise-step entries take it. */
int ldm_sampler_create_rflow(const float* coef_host, int n_steps, ldm_sampler** out) {
    if (!coef_host || n_steps < 1 || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    for (int k = 0; k < n_steps; ++k) {
        const float* r = coef_host + (size_t)k * 8;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[5])) return fail(LDM_ERR_BAD_ARG, "rectified-flow row %d is not finite", k);
    }
    std::unique_ptr<ldm_sampler> sp; LDM_TRY(sampler_alloc(coef_host, 8, n_steps, &sp));
    sp->kind = SAMPLER_RFLOW; sp->pred = PRED_EPSILON; sp->clip = 0;
    *out = sp.release();
    return 0;
}
/* Bytes of multistep state a step of n elements needs: 4 history slots, the saved sample and the accumulator, n floats each for a PNDM
 * sampler; n floats (the previous x0_hat) for a DPM-Solver++ sampler; 0 for DDPM / DDIM (and, with the error set, for a bad argument). */
size_t ldm_sampler_state_bytes(const ldm_sampler* sp, int64_t n) {
    if (!sp || n < 0) { fail(LDM_ERR_BAD_ARG, "bad argument"); return 0; }
    return sp->kind == SAMPLER_PNDM ? (size_t)n * 6 * sizeof(float) : sp->kind == SAMPLER_DPM ? (size_t)n * sizeof(float) : 0;
}
/* Hands a PNDM or DPM-Solver++ sampler its caller-owned device state buffer for steps of n elements (bytes >= ldm_sampler_state_bytes(sp, n)); it must
 * outlive every step (and every recorded graph replay) that uses it.  Nothing is allocated, zeroed or launched: the contents need no
 * initialisation.  Binding mid-chain loses the chain's history: reset first. */
int ldm_sampler_bind_state(ldm_sampler* sp, void* state, size_t bytes, int64_t n) {
    if (!sp || !state || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (!sampler_multistep(sp)) return fail(LDM_ERR_BAD_ARG, "only a PNDM or DPM-Solver++ sampler takes a state buffer");
    if ((uintptr_t)state % sizeof(float)) return fail(LDM_ERR_BAD_ARG, "state buffer not aligned to 4 bytes");
    const size_t need = ldm_sampler_state_bytes(sp, n);
    if (bytes < need) return fail(LDM_ERR_BAD_ARG, "state buffer of %zu bytes, %zu needed for %lld elements", bytes, need, (long long)n);
    sp->state = (float*)state; sp->state_n = n;
    return 0;
}
void ldm_sampler_destroy(ldm_sampler* sp) {
    if (!sp) return;
    if (sp->coef) (void)hipFree(sp->coef);
    if (sp->st) (void)hipFree(sp->st);
    delete sp;
}
/* step counter := 0, tbuf[0..B) := t of the first step.  PNDM: the history ring, the saved sample and the accumulator are addressed
 * through the step counter alone and row 0 reads none of them, so this rewinds the multistep state too; DPM-Solver++ likewise (row 0
 * does not read the previous x0_hat). */
int ldm_sampler_reset(ldm_sampler* sp, float* tbuf, int B, void* stream) {
    if (!sp || !tbuf || B < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(sampler_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sp->st, (const float*)sp->coef, tbuf, B);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* x := scheduler step (x, eps) for the step the device counter points at (in place), x0_out (optional) := x0_hat; then the counter
 * advances and tbuf[0..B) receives the next step's t.  Calls beyond n_steps leave x unchanged. */
int ldm_sampler_step(ldm_sampler* sp, const float* eps, float* x, float* x0_out, int64_t n, float* tbuf, int B, void* stream) {
    if (!sp || !eps || !x || !tbuf || n < 0 || B < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (sp->kind == SAMPLER_PNDM && eps == x) return fail(LDM_ERR_BAD_ARG, "PNDM: the model output may not alias x");
    if (sp->kind == SAMPLER_DPM && (eps == x || sp->state == x || sp->state == eps || (x0_out && (x0_out == x || x0_out == eps || x0_out == sp->state))))
        return fail(LDM_ERR_BAD_ARG, "DPM-Solver++: the model output, x, x0_out and the bound state may not alias");
    LDM_TRY(repaint_check(sp, n, B));
    LDM_TRY(sampler_launch(sp, eps, x, x0_out, n, tbuf, B, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
/* the N(0, 1) draws step `step` uses for a tensor of n elements (tests: statistics, reproducibility, fused == unfused) */
int ldm_sampler_noise(const ldm_sampler* sp, int step, float* out, int64_t n, void* stream) {
    if (!sp || !out || n < 0 || step < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (sp->kind == SAMPLER_RFLOW) return fail(LDM_ERR_BAD_ARG, "a rectified-flow sampler draws no noise");
    hipLaunchKernelGGL(sampler_noise_kernel, dim3(grid_for((n + 3) / 4, 256, 1024)), dim3(256), 0, (hipStream_t)stream, out, (long)n, step, sp->seed_lo, sp->seed_hi);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* One whole denoising step: eps_hat = UNet(x, tbuf) into eps_scratch, then ldm_sampler_step(x in place).  With
 * ldm_model_set_graph_mode the forward plan AND the scheduler step replay as ONE hipGraphLaunch: no host-side per-step work at all
 * (3d_ldm/inference.py:94-99's loop body). */
int ldm_unet_denoise_step(ldm_model* m, ldm_sampler* sp, float* x, int x_channels, const float* cond, int cond_channels,
                          float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!sp) return fail(LDM_ERR_BAD_ARG, "null sampler");
    if (m && m->type == 0 && x_channels != m->ucfg.out_channels) return fail(LDM_ERR_BAD_ARG, "x must have the UNet's out_channels (%d)", m->ucfg.out_channels);
    LDM_TRY(sampler_check_state(sp, (int64_t)B * x_channels * D * H * W));      // before the plan is built or anything is launched
    LDM_TRY(repaint_check(sp, (int64_t)B * x_channels * D * H * W, B));
    return unet_step(m, {x, x_channels, cond, cond_channels, tbuf, eps_scratch, B, B, D, H, W, workspace, workspace_bytes, stream, sp, x});
}

// ---- likelihood of a given latent (likelihood.h): MONAI's DiffusionInferer.get_likelihood as a device-resident loop -------------
// 16-byte vector access: whole quads per sample and every tensor aligned
static int lik_vec(int64_t per_sample, std::initializer_list<const void*> ptrs) {
    if (per_sample % 4) return 0;
    for (const void* q : ptrs) if ((uintptr_t)q % 16) return 0;
    return 1;
}
static int lik_check_shape(int B, int64_t per_sample) {
    if (B < 1 || B > 65535) return fail(LDM_ERR_BAD_ARG, "B must be in 1 .. 65535, got %d", B);
    if (per_sample < 1 || per_sample > ((int64_t)1 << 33)) return fail(LDM_ERR_BAD_ARG, "per_sample must be in 1 .. 2^33, got %lld", (long long)per_sample);
    return 0;
}
static int lik_check_row(const float* r, int k) {
    for (int j = 0; j < 8; ++j) if (!std::isfinite(r[j])) return fail(LDM_ERR_BAD_ARG, "likelihood row %d is not finite", k);
    if (!(r[0] > 0.f) || !(r[2] > 0.f) || !(r[4] > 0.f) || !(r[6] > 0.f) || r[5] < 0.f)
        return fail(LDM_ERR_BAD_ARG, "likelihood row %d: sqrt(abar), its reciprocal, 1/var and 1/sqrt(var) must be positive and t >= 0", k);
    return 0;
}
// the scratch of the term / finalize pair: [B][lik_blocks] doubles, then the B row indices the term kernel hands to the finalize kernel
static size_t lik_scratch_bytes(int B, int64_t per_sample) { return (size_t)B * lik_blocks((long)per_sample) * sizeof(double) + (size_t)B * sizeof(int); }
static void lik_launch(int pred, const LikParams& p, int k_host, int nb, int B, float* total, float* terms, SamplerState* st, int n_steps,
                       float* tbuf, hipStream_t s) {
    with_pred(pred, [&](auto P) { hipLaunchKernelGGL(lik_term_kernel<P()>, dim3(nb, B), dim3(LIK_THREADS), 0, s, p); });
    hipLaunchKernelGGL(lik_finalize_kernel, dim3(B), dim3(LIK_THREADS), 0, s, (const double*)p.partial, nb, (const int*)p.kk, k_host,
                       (double)p.per_sample, total, terms, B, st, p.coef, n_steps, tbuf);
}
static int likelihood_tail(const LikStep& ls, float* x_t, const float* m_out, float* tbuf, int B, int64_t per_sample, hipStream_t s) {
    const ldm_likelihood* lk = ls.lk;
    const int nb = lik_blocks((long)per_sample);
    LikParams p{}; p.x0 = ls.x0; p.xt = x_t; p.m = m_out; p.noise = lk->noise; p.map = ls.kl_map;
    p.partial = (double*)ls.scratch; p.kk = (int*)(p.partial + (size_t)B * nb);
    p.coef = lk->rows->coef; p.st = lk->rows->st; p.n_steps = lk->n_steps;
    p.per_sample = (long)per_sample; p.vec = lik_vec(per_sample, {ls.x0, x_t, m_out, lk->noise, ls.kl_map});
    p.clip = lk->clip; p.half_bin = lk->half_bin; p.seed_lo = lk->seed_lo; p.seed_hi = lk->seed_hi;
    lik_launch(lk->pred, p, 0, nb, B, ls.total, ls.terms, lk->rows->st, lk->n_steps, tbuf, s);
    return 0;
}
size_t ldm_likelihood_scratch_bytes(int B, int64_t per_sample) {
    if (lik_check_shape(B, per_sample)) return 0;
    return lik_scratch_bytes(B, per_sample);
}
/* coef_host = [n_steps][LDM_LIK_ROW] fp32 rows in scheduler.timesteps order (likelihood.h):
 * {sqrt(abar_t), sqrt(1 - abar_t), 1/sqrt(abar_t), c0, 1/var, t, 1/sqrt(var), c1, 0 ...}; the row with t == 0 scores the decoder term.
 * pred 0 epsilon, 1 sample, 2 v_prediction; clip: x0_hat is clamped to [-1, 1]; seed keys the Philox draw of z; bin_width > 0. */
int ldm_likelihood_create(const float* coef_host, int n_steps, int pred, int clip, uint64_t seed, float bin_width, ldm_likelihood** out) {
    static_assert(LIK_ROW == LDM_LIK_ROW, "row stride of the header");
    if (!coef_host || n_steps < 1 || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    if (!(bin_width > 0.f) || !std::isfinite(bin_width)) return fail(LDM_ERR_BAD_ARG, "bin_width must be positive");
    for (int k = 0; k < n_steps; ++k) LDM_TRY(lik_check_row(coef_host + (size_t)k * LIK_ROW, k));
    std::unique_ptr<ldm_sampler> rows; LDM_TRY(sampler_alloc(coef_host, LIK_ROW, n_steps, &rows));
    std::unique_ptr<ldm_likelihood> lk(new ldm_likelihood());
    lk->rows = rows.release(); lk->host.assign(coef_host, coef_host + (size_t)n_steps * LIK_ROW);
    lk->n_steps = n_steps; lk->pred = pred; lk->clip = clip ? 1 : 0; lk->half_bin = 0.5f * bin_width;
    lk->seed_lo = (unsigned)seed; lk->seed_hi = (unsigned)(seed >> 32);
    lk->next = n_steps;                               // no step before the first reset
    *out = lk.release();
    return 0;
}
void ldm_likelihood_destroy(ldm_likelihood* lk) {
    if (!lk) return;
    ldm_sampler_destroy(lk->rows);
    delete lk;
}
/* z as a tensor [B][per_sample]: what ldm_likelihood_reset / ldm_unet_likelihood_step draw when they are given no noise. */
int ldm_likelihood_noise(const ldm_likelihood* lk, float* out, int B, int64_t per_sample, void* stream) {
    if (!lk || !out) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(lik_check_shape(B, per_sample));
    hipLaunchKernelGGL(lik_noisy_kernel, dim3(lik_blocks((long)per_sample), B), dim3(LIK_THREADS), 0, (hipStream_t)stream, (const float*)nullptr,
                       (const float*)nullptr, out, (long)per_sample, lik_vec(per_sample, {out}), 0.f, 0.f, lk->seed_lo, lk->seed_hi);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The host-driven noising: x_t = row[0] x0 + row[1] noise, rounded as the device loop rounds it. */
int ldm_likelihood_noisy(const float* x0, const float* noise, const float* row, float* x_t, int B, int64_t per_sample, void* stream) {
    if (!x0 || !noise || !row || !x_t) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(lik_check_shape(B, per_sample));
    hipLaunchKernelGGL(lik_noisy_kernel, dim3(lik_blocks((long)per_sample), B), dim3(LIK_THREADS), 0, (hipStream_t)stream, x0, noise, x_t,
                       (long)per_sample, lik_vec(per_sample, {x0, noise, x_t}), row[0], row[1], 0u, 0u);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* Step counter := 0, total[0..B) := 0, x_t := noising of row 0 (z = noise, or the Philox draw where noise is NULL), tbuf[0..B) := t of
 * row 0.  The handle remembers `noise`: the steps that follow re-noise with the same z, so it must stay valid until the last step. */
int ldm_likelihood_reset(ldm_likelihood* lk, const float* x0, const float* noise, float* x_t, float* tbuf, int B, int64_t per_sample,
                         float* total, void* stream) {
    if (!lk || !x0 || !x_t || !tbuf || !total) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(lik_check_shape(B, per_sample));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(total, 0, (size_t)B * sizeof(float), s));
    hipLaunchKernelGGL(sampler_reset_kernel, dim3(1), dim3(64), 0, s, lk->rows->st, (const float*)lk->rows->coef, tbuf, B);
    hipLaunchKernelGGL(lik_noisy_kernel, dim3(lik_blocks((long)per_sample), B), dim3(LIK_THREADS), 0, s, x0, noise, x_t, (long)per_sample,
                       lik_vec(per_sample, {x0, noise, x_t}), lk->host[0], lk->host[1], lk->seed_lo, lk->seed_hi);
    HIP_TRY(hipGetLastError());
    lk->noise = noise; lk->next = 0;
    return 0;
}
/* The host-driven term of one timestep: the per-element terms of (x0, x_t, m) under `row` into kl_map (optional), their per-sample
 * mean into term_out[b] (optional) and added to total[b].  The device loop's per-element code and reduction, bit for bit. */
int ldm_likelihood_term(const float* x0, const float* x_t, const float* m, const float* row, int pred, int clip, float bin_width,
                        float* kl_map, float* term_out, float* total, int B, int64_t per_sample, void* scratch, size_t scratch_bytes,
                        void* stream) {
    if (!x0 || !x_t || !m || !row || !total || !scratch) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(lik_check_shape(B, per_sample));
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    if (!(bin_width > 0.f) || !std::isfinite(bin_width)) return fail(LDM_ERR_BAD_ARG, "bin_width must be positive");
    LDM_TRY(lik_check_row(row, 0));
    if ((uintptr_t)scratch % 8) return fail(LDM_ERR_BAD_ARG, "scratch not aligned to 8 bytes");
    if (scratch_bytes < lik_scratch_bytes(B, per_sample)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    const int nb = lik_blocks((long)per_sample);
    LikParams p{}; p.x0 = x0; p.xt = const_cast<float*>(x_t); p.m = m; p.map = kl_map; p.partial = (double*)scratch;
    p.c = lik_coef(row); p.per_sample = (long)per_sample; p.vec = lik_vec(per_sample, {x0, x_t, m, kl_map});
    p.clip = clip ? 1 : 0; p.half_bin = 0.5f * bin_width;
    lik_launch(pred, p, 0, nb, B, total, term_out, nullptr, 1, nullptr, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* One whole likelihood step on the row the device counter points at: m = UNet(x_t | cond, tbuf) into m_scratch, then the term kernel
 * (kl_map optional; x_t := the next row's noising in place) and the finalize kernel (total[b] += mean, terms[k][b] = mean where terms
 * [n_steps][B] is given, counter and tbuf advance).  The forward runs the tabulated-time-embedding plan where a sampler's step would.
 * Graph mode: ONE graph launch per step; the replay key holds the handle's never-reused id and every pointer.  A step past the last
 * row (or before the first reset): LDM_ERR_BAD_ARG, nothing launched. */
int ldm_unet_likelihood_step(ldm_model* m, ldm_likelihood* lk, const float* x0, float* x_t, int x_channels, const float* cond, int cond_channels,
                             float* tbuf, float* m_scratch, float* kl_map, float* terms, float* total, int B, int D, int H, int W,
                             void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!lk) return fail(LDM_ERR_BAD_ARG, "null likelihood handle");
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!x0 || !x_t || !tbuf || !m_scratch || !total || !scratch) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (D < 1 || H < 1 || W < 1) return fail(LDM_ERR_BAD_ARG, "bad shape");
    if (x_channels != m->ucfg.out_channels) return fail(LDM_ERR_BAD_ARG, "x_t must have the UNet's out_channels (%d)", m->ucfg.out_channels);
    const int64_t per_sample = (int64_t)x_channels * D * H * W;
    LDM_TRY(lik_check_shape(B, per_sample));
    if ((uintptr_t)scratch % 8) return fail(LDM_ERR_BAD_ARG, "scratch not aligned to 8 bytes");
    if (scratch_bytes < lik_scratch_bytes(B, per_sample)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    if (lk->next >= lk->n_steps) return fail(LDM_ERR_BAD_ARG, "likelihood step past the last row (%d rows): call ldm_likelihood_reset", lk->n_steps);
    const LikStep ls{lk, x0, kl_map, terms, total, scratch};
    LDM_TRY(unet_step(m, {x_t, x_channels, cond, cond_channels, tbuf, m_scratch, B, B, D, H, W, workspace, workspace_bytes, stream, lk->rows, x_t,
                          nullptr, &ls}));
    ++lk->next;
    return 0;
}
/* y [N][C][D][H][W] = nearest-neighbour resize of x [N][C][d][h][w] (fp32), PyTorch's index rule: src = min(floor(dst * (float)in / out), in - 1). */
int ldm_op_resize_nearest(const float* x, float* y, int N, int C, int d, int h, int w, int D, int H, int W, void* stream) {
    if (!x || !y) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (N < 1 || C < 1 || d < 1 || h < 1 || w < 1 || D < 1 || H < 1 || W < 1) return fail(LDM_ERR_BAD_ARG, "bad shape");
    const long total = (long)N * C * D * H * W;
    hipLaunchKernelGGL(resize_nearest_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, y, (long)N * C, d, h, w, D, H, W,
                       (float)d / (float)D, (float)h / (float)H, (float)w / (float)W);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- sliding-window sampling (window.h): a window grid over one full latent ---------------------------------------------------
/* dims, roi, n: [3]; starts: n[0] + n[1] + n[2] ints (axis after axis); weights: n[a] * roi[a] floats per axis (t_a[i][0..roi_a));
 * cover: 2 * dims[a] ints per axis ({first window, count} per position).  Everything is checked here: a window inside the volume,
 * starts ascending from 0 to dims - roi, every position covered by exactly the windows its cover entry names. */
int ldm_window_grid_create(const int* dims, const int* roi, const int* n, const int* starts, const float* weights, const int* cover,
                           ldm_window_grid** out) {
    if (!dims || !roi || !n || !starts || !weights || !cover || !out) return fail(LDM_ERR_BAD_ARG, "null argument");
    std::unique_ptr<ldm_window_grid> g(new ldm_window_grid());
    size_t ns = 0, nw = 0, nc = 0;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || roi[a] < 1 || roi[a] > dims[a] || n[a] < 1 || n[a] > dims[a])
            return fail(LDM_ERR_BAD_ARG, "window grid axis %d: dims %d, roi %d, %d windows", a, dims[a], roi[a], n[a]);
        g->dims[a] = dims[a]; g->roi[a] = roi[a]; g->n[a] = n[a];
        const int* st = starts + ns; const int* cv = cover + 2 * nc;
        if (st[0] != 0 || st[n[a] - 1] != dims[a] - roi[a]) return fail(LDM_ERR_BAD_ARG, "window grid axis %d: the windows must start at 0 and end flush", a);
        for (int i = 1; i < n[a]; ++i) if (st[i] <= st[i - 1]) return fail(LDM_ERR_BAD_ARG, "window grid axis %d: starts must ascend", a);
        for (int p = 0; p < dims[a]; ++p) {
            const int f = cv[2 * p], c = cv[2 * p + 1];
            if (f < 0 || c < 1 || f + c > n[a]) return fail(LDM_ERR_BAD_ARG, "window grid axis %d: bad cover entry at %d", a, p);
            for (int i = 0; i < n[a]; ++i) {
                const bool in = st[i] <= p && p < st[i] + roi[a];
                if (in != (i >= f && i < f + c)) return fail(LDM_ERR_BAD_ARG, "window grid axis %d: cover entry at %d disagrees with the starts", a, p);
            }
        }
        ns += n[a]; nw += (size_t)n[a] * roi[a]; nc += dims[a];
    }
    const size_t b_st = 0, b_w = (ns * 4 + 255) / 256 * 256, b_c = b_w + (nw * 4 + 255) / 256 * 256, bytes = b_c + nc * 8;
    HIP_TRY(hipMalloc((void**)&g->dev, bytes));
    hipError_t e = hipMemcpy(g->dev + b_st, starts, ns * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(g->dev + b_w, weights, nw * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(g->dev + b_c, cover, nc * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(g->dev); return fail(LDM_ERR_HIP, "window grid upload: %s", hipGetErrorString(e)); }
    size_t os = 0, ow = 0, oc = 0;
    for (int a = 0; a < 3; ++a) {
        g->geom.dim[a] = dims[a]; g->geom.roi[a] = roi[a]; g->geom.n[a] = n[a];
        g->geom.start[a] = (const int*)(g->dev + b_st) + os;
        g->geom.tab[a] = (const float*)(g->dev + b_w) + ow;
        g->geom.cover[a] = (const int2*)(g->dev + b_c) + oc;
        os += n[a]; ow += (size_t)n[a] * roi[a]; oc += dims[a];
    }
    *out = g.release();
    return 0;
}
void ldm_window_grid_destroy(ldm_window_grid* g) {
    if (!g) return;
    if (g->dev) { (void)hipDeviceSynchronize(); (void)hipFree(g->dev); }   // a replaying graph may still read the tables
    delete g;
}
static void window_gather_launch(const ldm_window_grid* g, const float* src, float* dst, int C, hipStream_t s) {
    hipLaunchKernelGGL(window_gather_kernel, dim3(grid_for(g->n_windows() * C * g->roi_vox(), 256, 2048)), dim3(256), 0, s, g->geom, src, dst, C);
}
/* dst [nW][C][roi] := the windows of src [C][dims] */
int ldm_window_gather(const ldm_window_grid* g, const float* src, float* dst, int C, void* stream) {
    if (!g || !src || !dst || C < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    window_gather_launch(g, src, dst, C, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* dst [C][dims] := sum over the windows covering each voxel of weight * src [nW][C][roi] */
int ldm_window_blend(const ldm_window_grid* g, const float* src, float* dst, int C, void* stream) {
    if (!g || !src || !dst || C < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(window_blend_kernel, dim3(grid_for(g->vox() * C, 256, 2048)), dim3(256), 0, (hipStream_t)stream, g->geom, src, dst, C);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* One whole windowed denoising step on the full latent x [x_channels][dims] (in place): the UNet on the windows xw [nW][x_channels][roi]
 * (with cond_w [nW][cond_channels][roi]) in chunks of `chunk` windows into eps_w [nW][out_channels][roi], then window_blend_step_kernel:
 * blend, scheduler step, and the new x written back into xw for the next step.  xw must hold the windows of x on entry (ldm_window_gather
 * once per chain; every step keeps it current).  tbuf: at least `chunk` entries.  Graph mode: the whole step is ONE graph launch. */
static int denoise_step_windows(ldm_model* m, ldm_sampler* sp, const ldm_window_grid* grid, float* x, int x_channels,
                                     const float* cond_w, int cond_channels, float* xw, float* eps_w, float* tbuf, int chunk,
                                     void* workspace, size_t workspace_bytes, void* stream, const Guide* guide) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!sp) return fail(LDM_ERR_BAD_ARG, "null sampler");
    if (!grid) return fail(LDM_ERR_BAD_ARG, "null window grid");
    if (!x || !xw || !eps_w || !tbuf) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (x_channels != m->ucfg.out_channels) return fail(LDM_ERR_BAD_ARG, "x must have the UNet's out_channels (%d)", m->ucfg.out_channels);
    if (!cond_w) cond_channels = 0;
    if (cond_channels < 0 || x_channels + cond_channels != m->ucfg.in_channels)
        return fail(LDM_ERR_BAD_ARG, "x channels (%d) + cond channels (%d) must equal the UNet's in_channels (%d)", x_channels, cond_channels, m->ucfg.in_channels);
    LDM_TRY(sampler_check_state(sp, grid->vox() * x_channels));
    LDM_TRY(repaint_check(sp, grid->vox() * x_channels, 1));
    const int64_t nw = grid->n_windows();
    if (chunk < 1 || chunk > nw) return fail(LDM_ERR_BAD_ARG, "chunk %d outside [1, %lld windows]", chunk, (long long)nw);
    return unet_step(m, {xw, x_channels, cond_w, cond_channels, tbuf, eps_w, chunk, nw, grid->roi[0], grid->roi[1], grid->roi[2],
                         workspace, workspace_bytes, stream, sp, x, guide, nullptr, grid});
}
int ldm_unet_denoise_step_windows(ldm_model* m, ldm_sampler* sp, const ldm_window_grid* grid, float* x, int x_channels,
                                  const float* cond_w, int cond_channels, float* xw, float* eps_w, float* tbuf, int chunk,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    return denoise_step_windows(m, sp, grid, x, x_channels, cond_w, cond_channels, xw, eps_w, tbuf, chunk, workspace, workspace_bytes, stream, nullptr);
}

/* Diagnostic builds only (EXTRA=-DLDM_KSTAMPS, tools/kstamps.py): the in-kernel stamps of the instrumented kernels, [entries][8] =
 * {kernel id, entry, stamp 1 ... stamp 6} in 10 ns ticks, in launch order; reset != 0 clears the log afterwards.  Returns the number
 * of entries (0 in the product library, which carries no stamps). */
int ldm_debug_kstamps(unsigned long long* out, int max_entries, int reset) {
#ifdef LDM_KSTAMPS
    if (!out || max_entries < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    unsigned n = 0;
    HIP_TRY(hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_kstamp_seq), sizeof n));
    const int cnt = (int)std::min<unsigned>(n, 8192u);
    const int take = std::min(cnt, max_entries);
    if (take > 0) HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kstamp), (size_t)take * 8 * sizeof(unsigned long long)));
    if (reset) { const unsigned z = 0; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_kstamp_seq), &z, sizeof z)); }
    return take;
#else
    (void)out; (void)max_entries; (void)reset;
    return 0;
#endif
}

/* Per-op timeline of every launch plan that runs from now on: a HIP event in front of every op, one CSV row per op appended to
 * `path` when the call returns (ops of the plan, op index, op kind, microseconds, shape); NULL or "" switches it off.  Tracing
 * synchronises at the end of every call and bypasses graph replay: a measurement aid, the hook behind the harness's --profile
 * (3d_ldm/train_autoencoder.py:81,312-329 wraps a few steps in torch.profiler).  Initial state: the LDM_PLAN_TRACE environment variable. */
int ldm_set_plan_trace(const char* path) {
    g_plan_trace.on = path && *path;
    g_plan_trace.path = g_plan_trace.on ? path : "";
    return 0;
}

/* on != 0: ldm_unet_forward replays a HIP graph of its launch plan whenever it sees the same (x, cond, timesteps, out,
 * workspace, stream) pointers again (callers keep those buffers fixed: the Python shell stages through persistent tensors).
 * Same kernels, same results; only the host cost per step changes (one graph launch instead of ~150 launches). */
int ldm_model_set_graph_mode(ldm_model* m, int on) {
    if (!m) return fail(LDM_ERR_BAD_ARG, "null model");
    m->graph_mode = on ? 1 : 0;
    if (!on) { for (auto& g : m->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec); m->graphs.clear(); }
    return 0;
}

/* Arithmetic of the INFERENCE plans (ldm_unet_forward, ldm_vae_encode, ldm_vae_decode and their *_taps forms):
 *   LDM_PREC_BF16 (0, default): bf16 storage, bf16 MFMA, fp32 accumulation (the headline path);
 *   LDM_PREC_FP32 (1): fp32 activations and weights on the fp32 matrix instruction (f32_path.h): the reference's own
 *   arithmetic (3d_ldm/train_diffusion.py:177: autocast off), within ~1e-5 rel-L2 of the CPU path instead of ~3e-2.
 * Switching to fp32 needs the parameters uploaded again (the unrounded copies are made at upload time): every ldm_model_load_*
 * call after the switch fills both arenas; forward calls fail with LDM_ERR_NOT_LOADED until then. */
int ldm_model_set_precision(ldm_model* m, int precision) {
    if (!m) return fail(LDM_ERR_BAD_ARG, "null model");
    if (precision != 0 && precision != 1) return fail(LDM_ERR_BAD_ARG, "precision must be LDM_PREC_BF16 (0) or LDM_PREC_FP32 (1)");
    if (precision == 1 && m->precision != 1) {          // every matrix must be uploaded again
        for (ParamDesc& d : m->params) d.loaded = false;
        m->loaded_count = 0;
    }
    m->precision = precision;
    return 0;
}
int ldm_model_get_precision(const ldm_model* m) { return m ? m->precision : -1; }

/* Debug taps: kind = "unet" | "enc" | "dec".  ldm_model_tap_count builds (and caches) the tapped plan of that shape and returns
 * the number of taps (or a negative status); ldm_model_tap_info describes tap i: name (block prefix in the MONAI state_dict),
 * dims = {B, C, D, H, W} and the element offset of its fp32 NCDHW tensor inside the taps_out / taps_in buffers of the
 * *_taps entry points (total elements = ldm_model_tap_elems). */
static const char* tap_kind(ldm_model* m, const char* kind) {
    if (!kind) return nullptr;
    if (m->type == 0) return strcmp(kind, "unet") == 0 ? "unet" : nullptr;
    return strcmp(kind, "enc") == 0 ? "enc" : strcmp(kind, "dec") == 0 ? "dec" : nullptr;
}
int ldm_model_tap_count(ldm_model* m, const char* kind, int B, int D, int H, int W) {
    if (!m || !tap_kind(m, kind)) return fail(LDM_ERR_BAD_ARG, "bad model / plan kind");
    std::shared_ptr<Plan> p; LDM_TRY(get_plan(m, tap_kind(m, kind), B, D, H, W, &p, 1));
    return (int)p->taps.size();
}
int64_t ldm_model_tap_elems(ldm_model* m, const char* kind, int B, int D, int H, int W) {
    if (!m || !tap_kind(m, kind)) return fail(LDM_ERR_BAD_ARG, "bad model / plan kind");
    std::shared_ptr<Plan> p; LDM_TRY(get_plan(m, tap_kind(m, kind), B, D, H, W, &p, 1));
    return (int64_t)p->tap_elems;
}
int ldm_model_tap_info(ldm_model* m, const char* kind, int B, int D, int H, int W, int i, char* name, int name_cap, int dims[5], int64_t* offset) {
    if (!m || !tap_kind(m, kind) || !name || name_cap < 1 || !dims || !offset) return fail(LDM_ERR_BAD_ARG, "bad argument");
    std::shared_ptr<Plan> p; LDM_TRY(get_plan(m, tap_kind(m, kind), B, D, H, W, &p, 1));
    if (i < 0 || i >= (int)p->taps.size()) return fail(LDM_ERR_BAD_ARG, "tap index out of range");
    const TapInfo& t = p->taps[i];
    snprintf(name, (size_t)name_cap, "%s", t.name.c_str());
    for (int k = 0; k < 5; ++k) dims[k] = t.dims[k];
    *offset = (int64_t)t.off;
    return 0;
}
/* ldm_unet_forward that also writes every block output to taps_out (fp32 NCDHW, layout from ldm_model_tap_info) and, when
 * taps_in is given, then OVERWRITES each block output with the caller's tensor, so that every block is computed from the
 * reference's input (teacher forcing: per-block parity without compounding rounding noise).  Eager launches only. */
int ldm_unet_forward_taps(ldm_model* m, const float* x, int x_channels, const float* cond, int cond_channels,
                          const float* timesteps, float* out, int B, int D, int H, int W, float* taps_out, const float* taps_in,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!x || !timesteps || !out || !taps_out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!cond) cond_channels = 0;
    std::shared_ptr<Plan> p; LDM_TRY(ready_plan(m, "unet", B, D, H, W, workspace, workspace_bytes, &p, taps_in ? 2 : 1));
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)x; bs.p[BASE_IO1] = (char*)cond; bs.p[BASE_IO2] = (char*)timesteps; bs.p[BASE_IO3] = (char*)out;
    bs.p[BASE_TAPO] = (char*)taps_out; bs.p[BASE_TAPI] = (char*)taps_in;
    const int rt[2] = {x_channels, cond_channels};
    LDM_TRY(ensure_derived(m, (hipStream_t)stream));
    return run_plan(*p, bs, rt, (hipStream_t)stream);
}
size_t ldm_model_taps_workspace_bytes(ldm_model* m, const char* kind, int B, int D, int H, int W, int force) {
    if (!m || !tap_kind(m, kind)) { fail(LDM_ERR_BAD_ARG, "bad model / plan kind"); return 0; }
    std::shared_ptr<Plan> p; if (get_plan(m, tap_kind(m, kind), B, D, H, W, &p, force ? 2 : 1)) return 0;
    return p->ws_bytes;
}

// ---- training: forward that keeps the tape, backward into one flat fp32 gradient buffer --------------------------
int64_t ldm_model_param_offset(const ldm_model* m, int i) {
    return (m && i >= 0 && i < (int)m->params.size()) ? m->params[i].flat_off : -1;
}

/* Re-pack every parameter from device fp32 tensors (MONAI layouts, library parameter order) into the bf16 arena:
 * what an optimizer step is followed by.  ptrs is a HOST array of n device pointers. */
int ldm_model_load_params_device(ldm_model* m, const float* const* ptrs, int n, void* stream) {
    if (!m || !ptrs) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (n != (int)m->params.size()) return fail(LDM_ERR_BAD_ARG, "expected %d parameter pointers, got %d", (int)m->params.size(), n);
    LDM_TRY(ensure_arena(m));
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k < n; ++k) {
        ParamDesc& d = m->params[k];
        if (!ptrs[k]) return fail(LDM_ERR_BAD_ARG, "parameter '%s': null pointer", d.name.c_str());
        if (d.kind == PK_VEC_F32) {
            HIP_TRY(hipMemcpyAsync(m->arena + d.dst_off, ptrs[k], (size_t)d.cout * 4, hipMemcpyDeviceToDevice, s));
        } else if (d.kind == PK_LINEAR_W) {
            hipLaunchKernelGGL(param_pack_kernel, dim3((d.cin + 63) / 64, d.cout), dim3(256), 0, s, ptrs[k], (bf16_t*)(m->arena + d.dst_off),
                               1, d.cout, d.cin, d.cin, d.cout, 0);
        } else {
            hipLaunchKernelGGL(param_pack_kernel, dim3((d.cin_s + 63) / 64, d.cout), dim3(256), 0, s, ptrs[k], (bf16_t*)(m->arena + d.dst_off),
                               d.k * d.k * d.k, d.cout, d.cin, d.cin_s, d.cout_pad, d.row_off);
        }
        if (m->precision == 1) { LDM_TRY(ensure_arena32(m)); pack32_device(m, d, ptrs[k], s); }
        if (!d.loaded) { d.loaded = true; m->loaded_count++; }
    }
    HIP_TRY(hipGetLastError());
    m->derived_dirty = true; m->temb_tab_valid = false;
    return 0;
}

/* The same from ONE flat fp32 device buffer holding every parameter at ldm_model_param_offset(i) (the layout of the flat
 * gradient buffer): a single descriptor-driven launch. */
static int ensure_pack_tab(ldm_model* m) {
    if (!m->pack_tab.nblocks) {
        std::vector<PackDesc> descs; std::vector<int2> map;
        for (const ParamDesc& d : m->params) {
            PackDesc e{}; e.src_off = (long)d.flat_off; e.dst_off = (long)d.dst_off;
            int nb;
            if (d.kind == PK_VEC_F32) { e.kind = 1; e.cout = d.cout; nb = (d.cout + 1023) / 1024; }
            else if (d.kind == PK_LINEAR_W) { e.kind = 0; e.taps = 1; e.cout = d.cout; e.cin = d.cin; e.cin_s = d.cin; e.cout_pad = d.cout; e.row_off = 0; nb = ((d.cin + 63) / 64) * d.cout; }
            else { e.kind = 0; e.taps = d.k * d.k * d.k; e.cout = d.cout; e.cin = d.cin; e.cin_s = d.cin_s; e.cout_pad = d.cout_pad; e.row_off = d.row_off; nb = ((d.cin_s + 63) / 64) * d.cout; }
            for (int b = 0; b < nb; ++b) map.push_back(make_int2((int)descs.size(), b));
            descs.push_back(e);
        }
        if (m->pack_tab.upload(descs, map) || m->pack_tab.ready()) return fail(LDM_ERR_HIP, "descriptor table upload failed");
    }
    return 0;
}

int ldm_model_load_params_flat(ldm_model* m, const float* flat, void* stream) {
    if (!m || !flat) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(ensure_arena(m));
    LDM_TRY(ensure_pack_tab(m));
    hipLaunchKernelGGL(param_pack_batched_kernel, dim3(m->pack_tab.nblocks), dim3(256), 0, (hipStream_t)stream,
                       (const PackDesc*)m->pack_tab.descs, (const int2*)m->pack_tab.map, flat, m->arena);
    if (m->precision == 1) {
        LDM_TRY(ensure_arena32(m));
        for (const ParamDesc& d : m->params) pack32_device(m, d, flat + d.flat_off, (hipStream_t)stream);
    }
    HIP_TRY(hipGetLastError());
    for (ParamDesc& d : m->params) if (!d.loaded) { d.loaded = true; m->loaded_count++; }
    m->derived_dirty = true; m->temb_tab_valid = false;
    return 0;
}

size_t ldm_unet_train_workspace_bytes(ldm_model* m, int B, int D, int H, int W) {
    if (!m || m->type != 0) { fail(LDM_ERR_BAD_ARG, "not a UNet handle"); return 0; }
    std::shared_ptr<Plan> p; if (get_plan(m, "train", B, D, H, W, &p)) return 0;
    return p->ws_bytes;
}

/* Same result as ldm_unet_forward; additionally leaves every activation, GroupNorm statistic and attention
 * log-sum-exp row in `workspace`, which must reach ldm_unet_train_backward untouched. */
int ldm_unet_train_forward(ldm_model* m, const float* x, int x_channels, const float* cond, int cond_channels,
                           const float* timesteps, float* out, int B, int D, int H, int W,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!x || !timesteps || !out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!cond) cond_channels = 0;
    std::shared_ptr<Plan> p; LDM_TRY(ready_plan(m, "train", B, D, H, W, workspace, workspace_bytes, &p));
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)x; bs.p[BASE_IO1] = (char*)cond; bs.p[BASE_IO2] = (char*)timesteps; bs.p[BASE_IO3] = (char*)out;
    const int rt[2] = {x_channels, cond_channels};
    m->train_cx = x_channels; m->train_cc = cond_channels;
    return run_plan(*p, bs, rt, (hipStream_t)stream, 0, p->bwd_begin);
}

/* grad_out: fp32 [B][out_channels][D][H][W] (dLoss/d eps_hat).  flat_grads: fp32 [ldm_model_param_numel_total], every
 * element is overwritten with dLoss/dparam (parameter i at ldm_model_param_offset(i), its MONAI tensor layout). */
int ldm_unet_train_backward(ldm_model* m, const float* grad_out, float* flat_grads, int B, int D, int H, int W,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!flat_grads) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    return ldm_unet_train_backward_input(m, grad_out, flat_grads, nullptr, nullptr, B, D, H, W, workspace, workspace_bytes, stream);
}

/* The backward of ldm_unet_train_forward with gradients w.r.t. the network input: dx fp32 [B][x_channels][D][H][W] and dcond
 * [B][cond_channels][D][H][W] (the channel counts of that forward call) are overwritten with dLoss/dx and dLoss/dcond; either may be
 * NULL.  flat_grads as above, or NULL: the data-only backward, which computes no bias, weight or time-embedding gradient, writes no
 * parameter gradient and exchanges nothing with other ranks.  All three NULL: LDM_ERR_BAD_ARG, nothing launched.  The three forms are
 * plans of their own over the forward's activations; size the workspace with ldm_unet_train_input_workspace_bytes. */
int ldm_unet_train_backward_input(ldm_model* m, const float* grad_out, float* flat_grads, float* dx, float* dcond,
                                  int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!grad_out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!flat_grads && !dx && !dcond) return fail(LDM_ERR_BAD_ARG, "no gradient requested: flat_grads, dx and dcond are all NULL");
    const bool input = dx || dcond;
    if (input && m->train_cx < 0) return fail(LDM_ERR_BAD_ARG, "input gradients before any ldm_unet_train_forward");
    if (dcond && m->train_cc < 1) return fail(LDM_ERR_BAD_ARG, "dcond given, but the forward had no condition tensor");
    std::shared_ptr<Plan> p;
    LDM_TRY(ready_plan(m, !input ? "train" : flat_grads ? "train_px" : "train_x", B, D, H, W, workspace, workspace_bytes, &p));
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)grad_out; bs.p[BASE_IO1] = (char*)dx; bs.p[BASE_IO2] = (char*)dcond; bs.p[BASE_IO4] = (char*)flat_grads;
    bs.in_cx = m->train_cx; bs.in_cc = m->train_cc;
    const int rt[2] = {m->ucfg.out_channels, 0};
    LaneCtx lanes;
    if (flat_grads) LDM_TRY(backward_lanes(m, (hipStream_t)stream, &lanes));
    return run_plan(*p, bs, rt, (hipStream_t)stream, p->bwd_begin, p->ops.size(), lanes);
}
/* Workspace that serves ldm_unet_train_forward and every form of ldm_unet_train_backward_input at this shape (the largest of the
 * three plans; ldm_unet_train_workspace_bytes is unchanged and serves callers that never ask for input gradients). */
size_t ldm_unet_train_input_workspace_bytes(ldm_model* m, int B, int D, int H, int W) {
    if (!m || m->type != 0) { fail(LDM_ERR_BAD_ARG, "not a UNet handle"); return 0; }
    size_t need = 0;
    for (const char* kind : {"train", "train_px", "train_x"}) {
        std::shared_ptr<Plan> p; if (get_plan(m, kind, B, D, H, W, &p)) return 0;
        need = std::max(need, p->ws_bytes);
    }
    return need;
}

size_t ldm_vae_train_workspace_bytes(ldm_model* m, int B, int D, int H, int W) {
    if (!m || m->type != 1) { fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle"); return 0; }
    std::shared_ptr<Plan> p; if (get_plan(m, "train", B, D, H, W, &p)) return 0;
    return p->ws_bytes;
}
/* AutoencoderKL.forward(x) -> (reconstruction, z_mu, z_sigma) with z = z_mu + z_sigma * eps, keeping the tape in `workspace`. */
int ldm_vae_train_forward(ldm_model* m, const float* x, const float* eps, float* recon, float* z_mu, float* z_sigma,
                          int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 1) return fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle");
    if (!x || !eps || !recon || !z_mu || !z_sigma) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    const int f = 1 << (m->vcfg.num_levels - 1);
    if (D % f || H % f || W % f) return fail(LDM_ERR_UNSUPPORTED, "image size must be a multiple of %d", f);
    std::shared_ptr<Plan> p; LDM_TRY(ready_plan(m, "train", B, D, H, W, workspace, workspace_bytes, &p));
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)x; bs.p[BASE_IO1] = (char*)eps; bs.p[BASE_IO2] = (char*)z_mu; bs.p[BASE_IO3] = (char*)z_sigma; bs.p[BASE_IO5] = (char*)recon;
    const int rt[2] = {m->vcfg.in_channels, 0};
    return run_plan(*p, bs, rt, (hipStream_t)stream, 0, p->bwd_begin);
}
/* d_recon: [B,Cout,D,H,W]; d_mu / d_sigma: [B,L,d,h,w] or NULL (the KL term's gradients); flat_grads as for the UNet. */
int ldm_vae_train_backward(ldm_model* m, const float* d_recon, const float* d_mu, const float* d_sigma, float* flat_grads,
                           int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 1) return fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle");
    if (!d_recon || !flat_grads) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    std::shared_ptr<Plan> p; LDM_TRY(ready_plan(m, "train", B, D, H, W, workspace, workspace_bytes, &p));
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)d_recon; bs.p[BASE_IO1] = (char*)d_mu; bs.p[BASE_IO2] = (char*)d_sigma; bs.p[BASE_IO4] = (char*)flat_grads;
    const int rt[2] = {m->vcfg.out_channels, 0};
    LaneCtx lanes;
    LDM_TRY(backward_lanes(m, (hipStream_t)stream, &lanes));
    return run_plan(*p, bs, rt, (hipStream_t)stream, p->bwd_begin, p->ops.size(), lanes);
}

/* AutoencoderKL.decode with gradients w.r.t. the latent (plan "dec_x"): the decoder half of the training plan, in its arithmetic, and a
 * data-only backward.  _forward: z [B][latent_channels][d][h][w] -> out [B][out_channels][d f][h f][w f], f = 2^(levels - 1), tape in
 * `workspace`, which must reach _backward untouched.  _backward: d_out (the shape of out) -> dz (the shape of z), overwritten.  No
 * parameter gradient is computed or written, nothing is exchanged with other ranks. */
static int vae_decode_grad_args(ldm_model* m, const void* a, const void* b, int B, int d, int h, int w) {
    if (!m || m->type != 1) return fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle");
    if (!a || !b) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || d < 1 || h < 1 || w < 1) return fail(LDM_ERR_BAD_ARG, "bad shape");
    return 0;
}
size_t ldm_vae_decode_grad_workspace_bytes(ldm_model* m, int B, int d, int h, int w) {
    if (!m || m->type != 1) { fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle"); return 0; }
    std::shared_ptr<Plan> p; if (get_plan(m, "dec_x", B, d, h, w, &p)) return 0;
    return p->ws_bytes;
}
int ldm_vae_decode_grad_forward(ldm_model* m, const float* z, float* out, int B, int d, int h, int w,
                                void* workspace, size_t workspace_bytes, void* stream) {
    LDM_TRY(vae_decode_grad_args(m, z, out, B, d, h, w));
    std::shared_ptr<Plan> p; LDM_TRY(ready_plan(m, "dec_x", B, d, h, w, workspace, workspace_bytes, &p));
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)z; bs.p[BASE_IO1] = (char*)out;
    const int rt[2] = {m->vcfg.latent_channels, 0};
    p->fwd_ran = true;
    return run_plan(*p, bs, rt, (hipStream_t)stream, 0, p->bwd_begin);
}
int ldm_vae_decode_grad_backward(ldm_model* m, const float* d_out, float* dz, int B, int d, int h, int w,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    LDM_TRY(vae_decode_grad_args(m, d_out, dz, B, d, h, w));
    std::shared_ptr<Plan> p; LDM_TRY(ready_plan(m, "dec_x", B, d, h, w, workspace, workspace_bytes, &p));
    if (!p->fwd_ran) return fail(LDM_ERR_BAD_ARG, "ldm_vae_decode_grad_backward before any ldm_vae_decode_grad_forward at this shape");
    Bases bs = model_bases(m, workspace);
    bs.p[BASE_IO0] = (char*)d_out; bs.p[BASE_IO1] = (char*)dz;
    bs.in_cx = m->vcfg.latent_channels; bs.in_cc = 0;
    const int rt[2] = {m->vcfg.out_channels, 0};
    return run_plan(*p, bs, rt, (hipStream_t)stream, p->bwd_begin, p->ops.size());
}

/* loss_out[0] = mean((pred - target)^2) over n fp32 elements; grad_out (optional, n elements) = 2 (pred - target) / n: the loss of
 * 3d_ldm/train_diffusion.py:207 and the gradient autograd hands to the network's backward (:214), in two launches. */
// reduction scratch of ldm_op_mse_loss / ldm_grad_sq_norm: one buffer per (device, entry point), allocated at the first call on
// that device (one process drives one GPU, but a caller with several devices current in turn must not get a foreign pointer);
// calls on the SAME device are expected on one stream at a time (include/ldm3d.h)
static float* device_scratch(int slot, size_t bytes) {
    static float* tab[32][3] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return nullptr;
    if (!tab[dev][slot] && hipMalloc((void**)&tab[dev][slot], bytes) != hipSuccess) tab[dev][slot] = nullptr;
    return tab[dev][slot];
}
int ldm_op_mse_loss(const float* pred, const float* target, int64_t n, float* loss_out, float* grad_out, void* stream) {
    if (!pred || !target || !loss_out || n < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    float* g_mse_parts = device_scratch(0, 1024 * 4);
    if (!g_mse_parts) return fail(LDM_ERR_HIP, "scratch allocation failed");
    const int nb = grid_for(n, 256 * 4, 1024);
    hipLaunchKernelGGL(mse_part_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred, target, (long)n, grad_out, g_mse_parts);
    hipLaunchKernelGGL(mse_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)g_mse_parts, nb, (long)n, loss_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ldm_grad_sq_norm(const float* flat_grads, int64_t n, float* out, void* stream) {
    if (!flat_grads || !out || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (((uintptr_t)flat_grads) & 15) return fail(LDM_ERR_BAD_ARG, "gradient buffer must be 16-byte aligned");
    float* g_norm_parts = device_scratch(1, 2048 * 4);
    if (!g_norm_parts) return fail(LDM_ERR_HIP, "scratch allocation failed");
    const int nb = grid_for((n + 3) / 4, 256, 2048);
    hipLaunchKernelGGL(sq_norm_part_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, flat_grads, (long)n, g_norm_parts);
    hipLaunchKernelGGL(sq_norm_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)g_norm_parts, nb, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
// Both optimizer entries and their EMA forms share one launcher each: ema == NULL instantiates the kernels without the EMA code.
static int adam_step_launch(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                            float beta1, float beta2, float eps, float weight_decay, int step, EmaCoef ek, const float* sq_norm,
                            float max_norm, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    AdamCoef k{lr, beta1, beta2, eps, 1.0f - powf(beta1, (float)step), sqrtf(1.0f - powf(beta2, (float)step)), max_norm, lr * weight_decay, step};
    const dim3 grid(grid_for(n, 256, 8192));
    if (ema) hipLaunchKernelGGL(adam_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq,
                                (long)n, k, sq_norm, ema, ek);
    else hipLaunchKernelGGL(adam_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq,
                            (long)n, k, sq_norm, (float*)nullptr, ek);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int model_adam_step_launch(ldm_model* m, float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                                  float* ema_flat, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                  EmaCoef ek, const float* sq_norm, float max_norm, void* stream) {
    if (!m || !params_flat || !grads_flat || !exp_avg || !exp_avg_sq || step < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    LDM_TRY(ensure_arena(m));
    LDM_TRY(ensure_pack_tab(m));
    AdamCoef k{lr, beta1, beta2, eps, 1.0f - powf(beta1, (float)step), sqrtf(1.0f - powf(beta2, (float)step)), max_norm, lr * weight_decay, step};
    const dim3 grid(m->pack_tab.nblocks);
    if (ema_flat) hipLaunchKernelGGL(adam_pack_batched_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream,
                                     (const PackDesc*)m->pack_tab.descs, (const int2*)m->pack_tab.map, params_flat, grads_flat, exp_avg,
                                     exp_avg_sq, m->arena, k, sq_norm, ema_flat, ek);
    else hipLaunchKernelGGL(adam_pack_batched_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream,
                            (const PackDesc*)m->pack_tab.descs, (const int2*)m->pack_tab.map, params_flat, grads_flat, exp_avg,
                            exp_avg_sq, m->arena, k, sq_norm, (float*)nullptr, ek);
    if (m->precision == 1) {
        LDM_TRY(ensure_arena32(m));
        for (const ParamDesc& d : m->params) pack32_device(m, d, params_flat + d.flat_off, (hipStream_t)stream);
    }
    HIP_TRY(hipGetLastError());
    for (ParamDesc& d : m->params) if (!d.loaded) { d.loaded = true; m->loaded_count++; }
    m->derived_dirty = true; m->temb_tab_valid = false;
    return 0;
}
// refused before any launch: no EMA buffer, or a decay outside [0, 1) (NaN fails the comparison too)
static int ema_args_ok(const float* ema, float ema_decay) {
    if (!ema) return fail(LDM_ERR_BAD_ARG, "null EMA buffer");
    if (!(ema_decay >= 0.f && ema_decay < 1.f)) return fail(LDM_ERR_BAD_ARG, "ema_decay must be in [0, 1), got %g", (double)ema_decay);
    return 0;
}

int ldm_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* sq_norm, float max_norm, void* stream) {
    return adam_step_launch(params, grads, exp_avg, exp_avg_sq, nullptr, n, lr, beta1, beta2, eps, weight_decay, step, EmaCoef{},
                            sq_norm, max_norm, stream);
}
int ldm_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, float ema_decay, int ema_warmup,
                      const float* sq_norm, float max_norm, void* stream) {
    LDM_TRY(ema_args_ok(ema, ema_decay));
    return adam_step_launch(params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, weight_decay, step,
                            EmaCoef{ema_decay, ema_warmup ? 1 : 0}, sq_norm, max_norm, stream);
}

/* The same optimizer step over the model's flat parameter buffer (layout of ldm_model_param_offset) that ALSO re-packs the bf16
 * arena from the updated values in the same pass: replaces ldm_adam_step + ldm_model_load_params_flat after it. */
int ldm_model_adam_step(ldm_model* m, float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, const float* sq_norm, float max_norm,
                        void* stream) {
    return model_adam_step_launch(m, params_flat, grads_flat, exp_avg, exp_avg_sq, nullptr, lr, beta1, beta2, eps, weight_decay, step,
                                  EmaCoef{}, sq_norm, max_norm, stream);
}
/* ... and keeps the EMA in ema_flat (same layout) like ldm_adam_step_ema; the arena is packed from the live weights, not the EMA. */
int ldm_model_adam_step_ema(ldm_model* m, float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                            float* ema_flat, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                            float ema_decay, int ema_warmup, const float* sq_norm, float max_norm, void* stream) {
    LDM_TRY(ema_args_ok(ema_flat, ema_decay));
    return model_adam_step_launch(m, params_flat, grads_flat, exp_avg, exp_avg_sq, ema_flat, lr, beta1, beta2, eps, weight_decay, step,
                                  EmaCoef{ema_decay, ema_warmup ? 1 : 0}, sq_norm, max_norm, stream);
}

static int vae_factor(const ldm_model* m) { return 1 << (m->vcfg.num_levels - 1); }

// The samples of an inference batch are independent (GroupNorm and attention are per sample), and the kernels address a tensor through
// buffer descriptors with 32-bit byte offsets: a batch whose largest activation would pass 4 GiB (4 x 64 ch x 160x224x160 in the fp32
// mode: 5.9 GB) runs as several sub-batches of the largest size that divides B and fits, one after the other on the same stream and
// in the same workspace.  Returns that sub-batch size and its plan.
static int vae_fit_batch(ldm_model* m, const char* kind, int B, int D, int H, int W, std::shared_ptr<Plan>* p, int* chunk) {
    int rc = 0;
    for (int c = B; c >= 1; --c) {
        if (B % c) continue;
        rc = get_plan(m, kind, c, D, H, W, p);
        if (rc == 0) { *chunk = c; return 0; }
        if (rc != LDM_ERR_UNSUPPORTED) break;
    }
    return rc;
}
size_t ldm_vae_encode_workspace_bytes(ldm_model* m, int B, int D, int H, int W) {
    if (!m || m->type != 1) { fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle"); return 0; }
    std::shared_ptr<Plan> p; int chunk = 0; if (vae_fit_batch(m, "enc", B, D, H, W, &p, &chunk)) return 0;
    return p->ws_bytes;
}
size_t ldm_vae_decode_workspace_bytes(ldm_model* m, int B, int d, int h, int w) {
    if (!m || m->type != 1) { fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle"); return 0; }
    std::shared_ptr<Plan> p; int chunk = 0; if (vae_fit_batch(m, "dec", B, d, h, w, &p, &chunk)) return 0;
    return p->ws_bytes;
}

static int vae_encode_impl(ldm_model* m, const float* x, const float* eps, float* z_mu, float* z_sigma, float* z,
                           int B, int D, int H, int W, float* taps_out, const float* taps_in, int tap_mode,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 1) return fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle");
    if (!x) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    const int f = vae_factor(m);
    if (D % f || H % f || W % f) return fail(LDM_ERR_UNSUPPORTED, "image size must be a multiple of %d", f);
    std::shared_ptr<Plan> p; int chunk = B;
    if (tap_mode) LDM_TRY(get_plan(m, "enc", B, D, H, W, &p, tap_mode)); else LDM_TRY(vae_fit_batch(m, "enc", B, D, H, W, &p, &chunk));
    LDM_TRY(check_ready(m, workspace, workspace_bytes, *p));
    LDM_TRY(ensure_derived(m, (hipStream_t)stream));
    const size_t in_n = (size_t)m->vcfg.in_channels * D * H * W, lat_n = (size_t)m->vcfg.latent_channels * (D / f) * (H / f) * (W / f);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        Bases bs = model_bases(m, workspace);
        auto at = [&](const float* q, size_t per) { return q ? (char*)(q + (size_t)b0 * per) : nullptr; };
        bs.p[BASE_IO0] = at(x, in_n); bs.p[BASE_IO1] = at(eps, lat_n); bs.p[BASE_IO2] = at(z_mu, lat_n); bs.p[BASE_IO3] = at(z_sigma, lat_n);
        bs.p[BASE_IO4] = at(z, lat_n);
        bs.p[BASE_TAPO] = (char*)taps_out; bs.p[BASE_TAPI] = (char*)taps_in;
        const int rt[2] = {m->vcfg.in_channels, 0};
        LDM_TRY(run_plan(*p, bs, rt, (hipStream_t)stream));
    }
    return 0;
}
int ldm_vae_encode(ldm_model* m, const float* x, const float* eps, float* z_mu, float* z_sigma, float* z,
                   int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    return vae_encode_impl(m, x, eps, z_mu, z_sigma, z, B, D, H, W, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}
/* ldm_vae_encode / ldm_vae_decode with debug taps (see ldm_unet_forward_taps) */
int ldm_vae_encode_taps(ldm_model* m, const float* x, const float* eps, float* z_mu, float* z_sigma, float* z,
                        int B, int D, int H, int W, float* taps_out, const float* taps_in,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!taps_out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    return vae_encode_impl(m, x, eps, z_mu, z_sigma, z, B, D, H, W, taps_out, taps_in, taps_in ? 2 : 1, workspace, workspace_bytes, stream);
}

static int vae_decode_impl(ldm_model* m, const float* z, float* out, int B, int d, int h, int w, float* taps_out, const float* taps_in,
                           int tap_mode, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 1) return fail(LDM_ERR_BAD_ARG, "not an AutoencoderKL handle");
    if (!z || !out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    std::shared_ptr<Plan> p; int chunk = B;
    if (tap_mode) LDM_TRY(get_plan(m, "dec", B, d, h, w, &p, tap_mode)); else LDM_TRY(vae_fit_batch(m, "dec", B, d, h, w, &p, &chunk));
    LDM_TRY(check_ready(m, workspace, workspace_bytes, *p));
    LDM_TRY(ensure_derived(m, (hipStream_t)stream));
    const int f = vae_factor(m);
    const size_t lat_n = (size_t)m->vcfg.latent_channels * d * h * w, out_n = (size_t)m->vcfg.out_channels * d * h * w * f * f * f;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        Bases bs = model_bases(m, workspace);
        bs.p[BASE_IO0] = (char*)(z + (size_t)b0 * lat_n); bs.p[BASE_IO1] = (char*)(out + (size_t)b0 * out_n);
        bs.p[BASE_TAPO] = (char*)taps_out; bs.p[BASE_TAPI] = (char*)taps_in;
        const int rt[2] = {m->vcfg.latent_channels, 0};
        LDM_TRY(run_plan(*p, bs, rt, (hipStream_t)stream));
    }
    return 0;
}
int ldm_vae_decode(ldm_model* m, const float* z, float* out, int B, int d, int h, int w,
                   void* workspace, size_t workspace_bytes, void* stream) {
    return vae_decode_impl(m, z, out, B, d, h, w, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}
int ldm_vae_decode_taps(ldm_model* m, const float* z, float* out, int B, int d, int h, int w, float* taps_out, const float* taps_in,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!taps_out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    return vae_decode_impl(m, z, out, B, d, h, w, taps_out, taps_in, taps_in ? 2 : 1, workspace, workspace_bytes, stream);
}

// ---- scheduler element-wise launches --------------------------------------------------------------------
int ldm_add_noise(const float* x0, const float* eps, const float* sqrt_a, const float* sqrt_b, float* out,
                  int B, int64_t per_sample, void* stream) {
    if (!x0 || !eps || !sqrt_a || !sqrt_b || !out || B < 1 || per_sample < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(add_noise_kernel, dim3(grid_for(per_sample * B)), dim3(256), 0, (hipStream_t)stream, x0, eps, sqrt_a, sqrt_b, out,
                       (long)per_sample, B);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The host-driven scheduler step (DDPMScheduler.step / DDIMScheduler.step) for a model of prediction type `pred` (0 epsilon, 1 sample,
 * 2 v_prediction), kind 0 = DDPM, 1 = DDIM: the device sampler's per-element step (sampler_update) with one sampler row (8 floats, as
 * ldm_sampler_create takes them) passed by value.  A null `noise` means sigma = 0. */
int ldm_scheduler_step(const float* model_out, const float* x, const float* noise, float* prev, float* x0_out, int64_t n, int kind, int pred,
                       const float* row, int clip, void* stream) {
    if (!model_out || !x || !prev || !row || n < 0 || kind < 0 || kind > 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    const SamplerCoef c{row[0], row[1], row[2], row[3], noise ? row[4] : 0.f, row[6], row[7]};
    const int cl = clip ? 1 : 0;
    const dim3 g(grid_for(n));
    hipStream_t s = (hipStream_t)stream;
    with_pred(pred, [&](auto P) { hipLaunchKernelGGL(scheduler_step_kernel<P()>, g, dim3(256), 0, s, model_out, x, noise, prev, x0_out, (long)n, c, kind, cl); });
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The host-driven PNDM step (PNDMScheduler.step): one row of the PNDM table by value (row: LDM_PNDM_ROW floats, as
 * ldm_sampler_create_pndm takes them) and the multistep state as explicit pointers; the device sampler's per-element arithmetic
 * (pndm_update), bit for bit.  prev := the step of (saved if the row uses the saved sample, else x) with model output m and the history
 * h1..h3 (latest first); acc_out := the row's accumulator update of acc_in (may alias).  A pointer the row does not use may be NULL;
 * one it uses may not.  The caller keeps the history list and the saved sample itself (the row's push / save bits are its business). */
int ldm_pndm_step(const float* m, const float* x, const float* h1, const float* h2, const float* h3, const float* saved,
                  const float* acc_in, float* acc_out, float* prev, int64_t n, int pred, const float* row, void* stream) {
    if (!m || !x || !prev || !row || n < 0 || prev == x || prev == m) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred != PRED_EPSILON && pred != PRED_V) return fail(LDM_ERR_BAD_ARG, "PNDM takes prediction type 0 (epsilon) or 2 (v_prediction), got %d", pred);
    const PndmCoef c = pndm_coef(row);
    const bool use_saved = (c.flags & PNDM_USE_SAVED) != 0, acc_rd = c.wacc != 0.f || (c.flags & PNDM_ACC_ADD), acc_wr = (c.flags & (PNDM_ACC_SET | PNDM_ACC_ADD)) != 0;
    if ((c.w1 != 0.f && !h1) || (c.w2 != 0.f && !h2) || (c.w3 != 0.f && !h3) || (use_saved && !saved) || (acc_rd && !acc_in) || (acc_wr && !acc_out))
        return fail(LDM_ERR_BAD_ARG, "PNDM step: the row reads or writes state that was passed as NULL");
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(grid_for(n));
    const float* sv = use_saved ? saved : nullptr; const float* ai = acc_rd ? acc_in : nullptr; float* ao = acc_wr ? acc_out : nullptr;
    const float* a1 = c.w1 != 0.f ? h1 : nullptr; const float* a2 = c.w2 != 0.f ? h2 : nullptr; const float* a3 = c.w3 != 0.f ? h3 : nullptr;
    with_pred<false>(pred, [&](auto P) { hipLaunchKernelGGL(pndm_step_kernel<P()>, g, dim3(256), 0, s, m, x, a1, a2, a3, sv, ai, ao, prev, (long)n, c); });
    HIP_TRY(hipGetLastError());
    return 0;
}
/* noisy = sqrt_a[b]*x0 + sqrt_b[b]*eps (skipped when noisy is NULL) and the regression target of prediction type `pred` in one pass:
 * eps (0), x0 (1) or the velocity sqrt_a[b]*eps - sqrt_b[b]*x0 (2). */
int ldm_add_noise_target(const float* x0, const float* eps, const float* sqrt_a, const float* sqrt_b, float* noisy, float* target,
                         int B, int64_t per_sample, int pred, void* stream) {
    if (!x0 || !eps || !sqrt_a || !sqrt_b || !target || B < 1 || per_sample < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    const dim3 g(grid_for(per_sample * B));
    hipStream_t s = (hipStream_t)stream;
    with_pred(pred, [&](auto P) { hipLaunchKernelGGL(add_noise_target_kernel<P()>, g, dim3(256), 0, s, x0, eps, sqrt_a, sqrt_b, noisy, target, (long)per_sample, B); });
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_scale(const float* x, float* y, int64_t n, float s, void* stream) {
    if (!x || !y || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, s);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The input side of a stage-2 training step from cached latents in one launch (latent_batch_kernel).  idx is a HOST array, read and
 * range-checked before the call returns and handed to the kernel by value; nothing is launched on a bad argument. */
static int latent_batch_impl(const float* mu_label, const float* sigma_label, const float* mu_image, const float* sigma_image, int N, int64_t per_sample,
                             const int* idx, int B, const float* sqrt_a, const float* sqrt_b, float scale, int pred, bool flow,
                             const float* e_label, const float* e_image, const float* noise, uint64_t seed, uint32_t step,
                             float* noisy, float* cond, float* target, float* draws_out, void* stream) {
    if (!mu_label || !sigma_label || !mu_image || !sigma_image || !idx || !sqrt_a || !sqrt_b || !noisy || !cond || !target)
        return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || B > LATENT_BATCH_MAX) return fail(LDM_ERR_BAD_ARG, "batch size %d outside 1 .. %d", B, LATENT_BATCH_MAX);
    if (N < 1 || per_sample < 1 || per_sample > ((int64_t)1 << 33)) return fail(LDM_ERR_BAD_ARG, "bad cache shape [%d][%lld]", N, (long long)per_sample);
    if (!flow && (pred < PRED_EPSILON || pred > PRED_V)) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    const bool draw = !e_label && !e_image && !noise;
    if (!draw && (!e_label || !e_image || !noise)) return fail(LDM_ERR_BAD_ARG, "e_label, e_image and noise are given together or all NULL");
    if (!draw && draws_out) return fail(LDM_ERR_BAD_ARG, "draws_out goes with device draws (e_label, e_image, noise all NULL)");
    LatentBatchParams p{};
    for (int b = 0; b < B; ++b) {
        if (idx[b] < 0 || idx[b] >= N) return fail(LDM_ERR_BAD_ARG, "idx[%d] = %d outside the cache's %d samples", b, idx[b], N);
        p.idx[b] = idx[b];
    }
    p.mu_l = mu_label; p.sg_l = sigma_label; p.mu_i = mu_image; p.sg_i = sigma_image; p.e_l = e_label; p.e_i = e_image; p.noise = noise;
    p.sa = sqrt_a; p.sb = sqrt_b; p.noisy = noisy; p.cond = cond; p.target = target; p.draws = draws_out;
    p.per_sample = (long)per_sample; p.B = B; p.scale = scale; p.scaled = scale != 1.0f;
    p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32); p.step = step;
    uintptr_t bits = 0;
    for (const void* q : {(const void*)mu_label, (const void*)sigma_label, (const void*)mu_image, (const void*)sigma_image, (const void*)e_label,
                          (const void*)e_image, (const void*)noise, (const void*)noisy, (const void*)cond, (const void*)target, (const void*)draws_out})
        bits |= (uintptr_t)q;
    p.vec = per_sample % 4 == 0 && (bits & 15) == 0;
    const dim3 g(grid_for((per_sample + 3) / 4 * B, 256, 1024));
    hipStream_t s = (hipStream_t)stream;
    if (flow) {
        if (draw) hipLaunchKernelGGL((latent_batch_kernel<PRED_FLOW, true>), g, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((latent_batch_kernel<PRED_FLOW, false>), g, dim3(256), 0, s, p);
    } else with_pred(pred, [&](auto P) {
        if (draw) hipLaunchKernelGGL((latent_batch_kernel<P(), true>), g, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((latent_batch_kernel<P(), false>), g, dim3(256), 0, s, p);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_latent_batch(const float* mu_label, const float* sigma_label, const float* mu_image, const float* sigma_image, int N, int64_t per_sample,
                     const int* idx, int B, const float* sqrt_a, const float* sqrt_b, float scale, int pred,
                     const float* e_label, const float* e_image, const float* noise, uint64_t seed, uint32_t step,
                     float* noisy, float* cond, float* target, float* draws_out, void* stream) {
    return latent_batch_impl(mu_label, sigma_label, mu_image, sigma_image, N, per_sample, idx, B, sqrt_a, sqrt_b, scale, pred, false,
                             e_label, e_image, noise, seed, step, noisy, cond, target, draws_out, stream);
}
/* ldm_latent_batch for a rectified-flow model (RFlowScheduler): one_minus_tau / tau [B] stand where sqrt_a / sqrt_b stand there
 * (ldm_rflow_timesteps writes them), the noisy latent is rounded the same way and target = z - noise; the draws, their keys, the
 * unscaled condition and every refusal are ldm_latent_batch's. */
int ldm_latent_batch_rflow(const float* mu_label, const float* sigma_label, const float* mu_image, const float* sigma_image, int N, int64_t per_sample,
                           const int* idx, int B, const float* one_minus_tau, const float* tau, float scale,
                           const float* e_label, const float* e_image, const float* noise, uint64_t seed, uint32_t step,
                           float* noisy, float* cond, float* target, float* draws_out, void* stream) {
    return latent_batch_impl(mu_label, sigma_label, mu_image, sigma_image, N, per_sample, idx, B, one_minus_tau, tau, scale, 0, true,
                             e_label, e_image, noise, seed, step, noisy, cond, target, draws_out, stream);
}
/* The host-driven rectified-flow step (RFlowScheduler.step): prev = x + row[0] m, x0_out (optional) = x + row[1] m with one sampler row
 * (8 floats, as ldm_sampler_create_rflow takes them) by value; the device sampler's per-element arithmetic (flow_update), bit for bit.
 * prev may alias x. */
int ldm_rflow_step(const float* m, const float* x, float* prev, float* x0_out, int64_t n, const float* row, void* stream) {
    if (!m || !x || !prev || !row || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (x0_out && (x0_out == x || x0_out == m || x0_out == prev)) return fail(LDM_ERR_BAD_ARG, "x0_out may not alias another tensor of the step");
    if (prev == m) return fail(LDM_ERR_BAD_ARG, "prev may not alias the model output");
    const FlowCoef c{row[0], row[1]};
    hipLaunchKernelGGL(flow_step_kernel<>, dim3(grid_for((n + 3) / 4, 256, 1024)), dim3(256), 0, (hipStream_t)stream, m, x, prev, x0_out, (long)n, c);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* noisy = a[b]*x0 + b[b]*noise (skipped when noisy is NULL; a = 1 - tau, b = tau: RFlowScheduler.add_noise) and the velocity target
 * x0 - noise in one pass.  noisy rounds as ldm_add_noise rounds launches of at most 2^20 elements: both products, then the sum. */
int ldm_rflow_noise_target(const float* x0, const float* noise, const float* a, const float* b, float* noisy, float* target,
                           int B, int64_t per_sample, void* stream) {
    if (!x0 || !noise || !a || !b || !target || B < 1 || per_sample < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    uintptr_t bits = 0;
    for (const void* q : {(const void*)x0, (const void*)noise, (const void*)noisy, (const void*)target}) bits |= (uintptr_t)q;
    const int vec = per_sample % 4 == 0 && (bits & 15) == 0;
    hipLaunchKernelGGL(rflow_noise_target_kernel<>, dim3(grid_for((per_sample + 3) / 4 * B, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       x0, noise, a, b, noisy, target, (long)per_sample, B, vec);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The per-sample scalars of a rectified-flow training step in one launch (RFlowScheduler.sample_timesteps and the coefficients of its
 * add_noise): t [B] (the UNet's timestep input), one_minus_tau [B] and tau [B], device fp32.  method 0 uniform (t = u T), 1 logit-normal
 * (t = sigmoid(loc + scale n) T); discrete floors t; transform_ratio r != 0 then maps t to T r s / (1 + (r - 1) s), s = t / T.  draw [B]
 * (device; u or n) or NULL: drawn by Philox4x32-10(counter = (0, idx[b], step, 0x1a7e0000 + 3), key = seed), a stream beside the three of
 * ldm_latent_batch.  idx is a HOST array read before the call returns (only with draw NULL; NULL then means 0 .. B-1). */
int ldm_rflow_timesteps(const int* idx, int B, int T, int method, float loc, float scale, int discrete, float transform_ratio,
                        const float* draw, uint64_t seed, uint32_t step, float* t, float* one_minus_tau, float* tau, void* stream) {
    if (!t || !one_minus_tau || !tau) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || B > LATENT_BATCH_MAX) return fail(LDM_ERR_BAD_ARG, "batch size %d outside 1 .. %d", B, LATENT_BATCH_MAX);
    if (method != RFLOW_UNIFORM && method != RFLOW_LOGIT_NORMAL) return fail(LDM_ERR_BAD_ARG, "unknown sample method %d (0 uniform, 1 logit-normal)", method);
    if (T < 1) return fail(LDM_ERR_BAD_ARG, "num_train_timesteps %d < 1", T);
    if (method == RFLOW_LOGIT_NORMAL && !(scale > 0.f && std::isfinite(scale) && std::isfinite(loc)))
        return fail(LDM_ERR_BAD_ARG, "logit-normal: scale must be positive and loc finite");
    if (!(transform_ratio >= 0.f) || !std::isfinite(transform_ratio)) return fail(LDM_ERR_BAD_ARG, "transform ratio must be positive (0 = off)");
    RflowTimestepParams p{};
    for (int b = 0; b < B; ++b) p.idx[b] = idx ? idx[b] : b;
    p.draw = draw; p.t = t; p.one_minus_tau = one_minus_tau; p.tau = tau; p.B = B; p.method = method; p.discrete = discrete ? 1 : 0;
    p.T = (float)T; p.loc = loc; p.scale = scale; p.ratio = transform_ratio;
    p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32); p.step = step;
    hipLaunchKernelGGL(rflow_timesteps_kernel<>, dim3(1), dim3(LATENT_BATCH_MAX), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- profiling: HIP events around every launch of one conv tile configuration ------------------------------
int ldm_profile_start(int wgm, int wgn, int bk, int max_launches) {
    if (max_launches < 1) return fail(LDM_ERR_BAD_ARG, "max_launches < 1");
    for (auto e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof = ProfState();
    g_prof.ev.resize((size_t)max_launches * 2);
    for (auto& e : g_prof.ev) HIP_TRY(hipEventCreate(&e));
    g_prof.wgm = wgm; g_prof.wgn = wgn; g_prof.bk = bk & 0xff; g_prof.halo = (bk >> 8) & 1; g_prof.on = true;   // bk | 256 selects conv3_halo_kernel
    return 0;
}
/* Per-launch view of the instrumented launches, to be called BEFORE ldm_profile_stop (which frees the events): fills
 * flops[k] / ms[k] for k < min(n, max) and returns n (the number of instrumented launches) or a negative status. */
int ldm_profile_detail(double* flops, double* ms, int max) {
    if (!flops || !ms || max < 0) return fail(LDM_ERR_BAD_ARG, "null argument");
    const int n = (int)(g_prof.used / 2);
    for (int k = 0; k < n && k < max; ++k) {
        HIP_TRY(hipEventSynchronize(g_prof.ev[2 * k + 1]));
        float t = 0.f; HIP_TRY(hipEventElapsedTime(&t, g_prof.ev[2 * k], g_prof.ev[2 * k + 1]));
        flops[k] = g_prof.flops[k]; ms[k] = t;
    }
    return n;
}
/* out[0] = instrumented launches, out[1] = their total ms, out[2] = their total algorithmic FLOPs,
 * out[3] = all conv launches seen, out[4] = algorithmic FLOPs of all conv launches seen */
int ldm_profile_stop(double out[5]) {
    if (!out) return fail(LDM_ERR_BAD_ARG, "null out");
    g_prof.on = false;
    double ms = 0.0, fl = 0.0;
    for (size_t k = 0; k + 1 < g_prof.used + 1 && k < g_prof.used; k += 2) {
        HIP_TRY(hipEventSynchronize(g_prof.ev[k + 1]));
        float t = 0.f; HIP_TRY(hipEventElapsedTime(&t, g_prof.ev[k], g_prof.ev[k + 1]));
        ms += t; fl += g_prof.flops[k / 2];
    }
    out[0] = (double)(g_prof.used / 2); out[1] = ms; out[2] = fl; out[3] = (double)g_prof.launches_all; out[4] = g_prof.flops_all;
    for (auto e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear(); g_prof.used = 0; g_prof.flops.clear();
    return 0;
}
/* Tile configuration the planner chose for each conv of a cached plan: fills cfgs[4*i..] = {wgm, wgn, bk | halo << 8, splitk} */
int ldm_model_plan_conv_cfgs(ldm_model* m, const char* kind, int B, int D, int H, int W, int* cfgs, int max_convs) {
    if (!m || !kind) return fail(LDM_ERR_BAD_ARG, "null argument");
    std::shared_ptr<Plan> p; LDM_TRY(get_plan(m, kind, B, D, H, W, &p));
    int n = 0;
    for (const Op& o : p->ops) if (o.kind == OP_CONV) {
        if (cfgs && n < max_convs) { cfgs[4 * n] = o.cc.wgm; cfgs[4 * n + 1] = o.cc.wgn; cfgs[4 * n + 2] = o.cc.bk | ((o.cc.cube ? 5 : o.cc.plane ? 6 : o.cc.halo) << 8); cfgs[4 * n + 3] = o.cc.splitk; }   // cube: halo code 5, plane: 6
        ++n;
    } else if (o.kind == OP_CONV_BLOCK) {            // conv3_block_kernel: reported as a 4 x 1 tile, 32-channel chunks, halo = 3
        if (cfgs && n < max_convs) { cfgs[4 * n] = 4; cfgs[4 * n + 1] = o.cv.couts == 128 ? 2 : 1; cfgs[4 * n + 2] = 32 | ((o.cv.couts == 128 ? 4 : 3) << 8); cfgs[4 * n + 3] = 1; }
        ++n;
    }
    return n;
}

/* Launches of a cached inference plan ("unet" | "enc" | "dec"; builds it if needed): the number of ops. */
int ldm_model_plan_launches(ldm_model* m, const char* kind, int B, int D, int H, int W) {
    if (!m || !kind) return fail(LDM_ERR_BAD_ARG, "null argument");
    std::shared_ptr<Plan> p; LDM_TRY(get_plan(m, kind, B, D, H, W, &p));
    int n = 0;
    for (const Op& o : p->ops) if (o.kind != OP_TAP) ++n;
    return n;
}

// ---- operator-level entry points (the same kernels the plans launch; used by per-kernel parity tests and
//      micro-benchmarks).  Tensors are NDHWC bf16 device memory with C % 32 == 0. -------------------------------
static char* g_zero_page = nullptr;
static int ensure_zero_page() {
    if (g_zero_page) return 0;
    HIP_TRY(hipMalloc((void**)&g_zero_page, 8192));
    HIP_TRY(hipMemset(g_zero_page, 0, 8192));
    HIP_TRY(hipDeviceSynchronize());                 // see ensure_arena
    return 0;
}

// stats (optional): GroupNorm partial slabs of the bf16 output, exactly as the plans request them from the producing kernel;
// *stats_nrb receives the slab rows per sample.  With stats the split-K finalize is the write-through variant the plans launch.
/* 3x3x3 stride-1 pad-1 convolution with 64 output channels as conv3_block_kernel (conv_block.h; the plans pick it for the AutoencoderKL's
 * full-resolution level): x [N][D][H][W][cin] bf16, w packed [27][64][cin] bf16, out [N*D*H*W][64] bf16; bias [64], temb [N][temb_stride],
 * residual [N*D*H*W][64] optional.  stats (optional): [N * rows][64][2] per-block (sum, sum of squares) of the stored values,
 * rows = ldm_op_conv3d_block_stats_rows(D, H, W, th); th = 8 (4 x 8 x 16 blocks) or 4 (4 x 4 x 16). */
/* The same for 128 output channels (conv3_block128_kernel): w packed [27][128][cin], out / residual [N*D*H*W][128], bias [128],
 * stats [N * ldm_op_conv3d_block_stats_rows(D, H, W, 8)][128][2]. */
static int op_conv3d_block(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                           void* out, float* stats, int N, int D, int H, int W, int th, void* stream) {   // th 0: conv3_block128_kernel
    if (!x || !w || !out || N < 1 || D < 1 || H < 1 || W < 1 || cin < 32 || cin % 32 || (th != 0 && th != 4 && th != 8)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if ((long)N * D * H * W * cin * 2 >= (1L << 32)) return fail(LDM_ERR_BAD_ARG, "the input tensor exceeds 4 GiB (split the batch)");
    BlockParams q{}; q.x = (const bf16_t*)x; q.w = (const bf16_t*)w; q.bias = bias; q.temb = temb; q.temb_stride = temb_stride;
    q.residual = (const bf16_t*)residual; q.out = (bf16_t*)out; q.stats = stats; q.N = N; q.D = D; q.H = H; q.W = W; q.Cin = cin;
    HIP_TRY(th ? launch_conv_block(q, th, (hipStream_t)stream) : launch_conv_block128(q, (hipStream_t)stream));
    return 0;
}
int ldm_op_conv3d_block128(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                           void* out, float* stats, int N, int D, int H, int W, void* stream) {
    return op_conv3d_block(x, cin, w, bias, temb, temb_stride, residual, out, stats, N, D, H, W, 0, stream);
}
/* tests only: the grid of conv3_block_kernel's tile loop (0 = two workgroups per CU); returns the previous value */
int ldm_debug_conv_block_slots(int slots) {
#ifdef LDM_EXPERIMENTS
    const int old = g_block_slots; g_block_slots = slots < 0 ? 0 : slots; return old;
#else
    (void)slots; return -1;                              // the tile-loop form of conv3_block_kernel is not in the product library
#endif
}
int ldm_op_conv3d_block_stats_rows(int D, int H, int W, int th) {
    if (th != 4 && th != 8) return 0;
    return ((D + BLK_TD - 1) / BLK_TD) * ((H + th - 1) / th) * ((W + BLK_TW - 1) / BLK_TW);
}
int ldm_op_conv3d_block(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                        void* out, float* stats, int N, int D, int H, int W, int th, void* stream) {
    if (th != 4 && th != 8) return fail(LDM_ERR_BAD_ARG, "bad argument");
    return op_conv3d_block(x, cin, w, bias, temb, temb_stride, residual, out, stats, N, D, H, W, th, stream);
}

static int op_conv3d_impl(const void* xa, int ca, const void* xb, int cb, const void* w, const float* bias,
                          const void* x1a, int c1a, const void* x1b, int c1b, const void* w1, const float* bias2,
                          const float* temb, int temb_stride, const void* residual, void* out_bf16, float* out_f32,
                          int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups,
                          int cout, int cout_pad, int wgn, int splitk, void* scratch, size_t scratch_bytes, void* stream,
                          float* stats, int* stats_nrb, FinGnParams* fg = nullptr) {
    if (!xa || !w || (!out_bf16 && !out_f32 && !fg)) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!xb) cb = 0;
    if (!x1a) { c1a = 0; c1b = 0; }
    if (!x1b) c1b = 0;
    const int cin0 = ca + cb, cin1 = c1a + c1b;
    // zero padding reads come from the 8 KiB zero page: at most 4096 channels per source row for a padded conv (1x1 GEMMs have none)
    const int cmax = (ksize == 1 && stride == 1 && pad == 0 && ups == 0) ? 65536 : 4096;
    if (ca % 32 || cb % 32 || c1a % 32 || c1b % 32 || cout_pad % 64 || cout > cout_pad || cin0 > cmax || cin1 > 4096)
        return fail(LDM_ERR_BAD_ARG, "channel counts must be multiples of 32 (cout_pad of 64), at most %d per row", cmax);
    if (ksize != 1 && ksize != 3) return fail(LDM_ERR_UNSUPPORTED, "ksize must be 1 or 3");
    int exact = 0;
    if (ups == 2) { ups = 1; exact = 1; }            // ups = 2: zero-insertion upsample (transposed stride-2 conv)
    if (ups < 0 || ups > 1 || stride < 1 || stride > 2) return fail(LDM_ERR_UNSUPPORTED, "stride 1|2, ups 0|1|2");
    LDM_TRY(ensure_zero_page());
    int bk = 64;
    if (ca % 64 || cb % 64 || c1a % 64 || c1b % 64) bk = 32;
    const int Do = conv_out_size(Din, ksize, stride, pad, ups), Ho = conv_out_size(Hin, ksize, stride, pad, ups), Wo = conv_out_size(Win, ksize, stride, pad, ups);
    const long M = (long)N * Do * Ho * Wo;
    if (M >= (1L << 31) || M < 1) return fail(LDM_ERR_BAD_ARG, "bad output size");
    if (!stats && !wgn && !splitk && out_bf16 && !out_f32 && gemm_light_ok(ksize, stride, ups, cin0, cin1 == 0, !temb && !bias2) &&
        Builder::light_enabled() && M * (long)cin0 * 2 < (1L << 31)) {
        LightParams lp{}; lp.x = (const bf16_t*)xa; lp.w = (const bf16_t*)w; lp.bias = bias; lp.residual = (const bf16_t*)residual;
        lp.out = (bf16_t*)out_bf16; lp.stats = nullptr; lp.M = (int)M; lp.K = cin0; lp.CoutS = rup(cout, 32);
        lp.xb = (const bf16_t*)xb; lp.ca = ca;
        HIP_TRY(launch_gemm_1x1(lp, cout_pad, gemm_light_big(M, cout_pad), gemm_wg_ok(cb == 0, cin0, M), (hipStream_t)stream));
        return 0;
    }
    if ((wgn && wgn != 1 && wgn != 2 && wgn != 4) || (wgn && cout_pad % (64 * wgn))) return fail(LDM_ERR_BAD_ARG, "bad wgn");
    if (splitk < 0 || splitk > ksize * ksize * ksize * (cin0 / bk) + cin1 / bk) return fail(LDM_ERR_BAD_ARG, "bad splitk");
    // the geometry of a plan's record; the configuration and every derived integer come from the functions the plans use
    ConvRec c{}; c.N = N; c.Din = Din; c.Hin = Hin; c.Win = Win; c.Dout = Do; c.Hout = Ho; c.Wout = Wo;
    c.k = ksize; c.stride = stride; c.pad = pad; c.ups = ups; c.exact = exact; c.M = (int)M;
    c.couts = rup(cout, 32); c.cout_pad = cout_pad; c.cout_real = cout; c.ca = ca; c.cb = cb; c.c1a = c1a; c.c1b = c1b; c.temb_stride = temb_stride;
    // no forced tile shape or split: conv3_cube_kernel / conv3_plane_kernel where the plans would take them
    const bool small = !wgn && !splitk && !out_f32 && !ldm_xknob("LDM_CONV_DBG", 0) && Builder::halo_enabled();
    ConvCfg cc = Builder::pick_cfg(c, bk, small, small && out_bf16 && !fg, wgn, splitk);
    c.nchunk0 = cin0 / cc.bk; c.nchunk1 = cin1 / cc.bk;
    if (fg && cc.splitk > 1) cc.slab_lg = fg->lg;    // planar slabs for the group-owning finalize
    ConvParams p = conv_params_geom(c, cc);
    p.x0a = (const bf16_t*)xa; p.x0b = (const bf16_t*)xb; p.w0 = (const bf16_t*)w;
    p.x1a = (const bf16_t*)x1a; p.x1b = (const bf16_t*)x1b; p.w1 = (const bf16_t*)w1;
    p.zero_page = (const bf16_t*)g_zero_page;
    p.bias = bias; p.bias2 = bias2; p.temb = temb; p.residual = (const bf16_t*)residual;
    p.out = out_f32 ? nullptr : (bf16_t*)out_bf16; p.out_f32 = out_f32;
    if (cc.splitk > 1) {
        const size_t need = (size_t)cc.splitk * M * cout_pad * 4;
        if (!scratch || scratch_bytes < need) return fail(LDM_ERR_WORKSPACE, "split-K scratch too small: need %zu bytes", need);
        p.partial = (float*)scratch;
    }
    if (stats) {                                     // the rows a plan's GroupNorm would find behind this conv (conv_stats_rows)
        if (out_f32 || !stats_nrb) return fail(LDM_ERR_BAD_ARG, "statistics need the bf16 output form");
        *stats_nrb = conv_stats_rows(c, cc);
        if (*stats_nrb < 1) return fail(LDM_ERR_UNSUPPORTED, "statistics: tiles (split-K: 32-row blocks) straddle samples");
        p.stats = stats;
    }
    p.dbg = (int)ldm_xknob("LDM_CONV_DBG", 0);
    if (p.dbg & 512) {                          // diagnostic stamps go to the caller's scratch (needs nwg * 64 bytes)
        if (cc.splitk > 1 || !scratch || scratch_bytes < (size_t)p.mtiles * p.ntiles * (64 + 4096)) return fail(LDM_ERR_BAD_ARG, "stamps need scratch and splitk 1");
        p.stamps = (unsigned long long*)scratch;
    }
    LDM_TRY(launch_conv(p, cc, (hipStream_t)stream));
    if (cc.splitk > 1) {
        const FinalizeParams f = finalize_params(p);
        if (fg) {                                    // finalize + GroupNorm in one launch (fin_gn.h), as the plans' OP_FIN_GN
            fg->f = f; fg->f.stats = nullptr;
            HIP_TRY(launch_fin_gn(*fg, N, wt_stores(), (hipStream_t)stream));
        } else
            launch_finalize(f, stats && wt_stores(), (hipStream_t)stream);
    } else if (fg) return fail(LDM_ERR_UNSUPPORTED, "the fused finalize + GroupNorm needs a conv that is split over K");
    HIP_TRY(hipGetLastError());
    return 0;
}

int ldm_op_conv3d(const void* xa, int ca, const void* xb, int cb, const void* w, const float* bias,
                  const void* x1a, int c1a, const void* x1b, int c1b, const void* w1, const float* bias2,
                  const float* temb, int temb_stride, const void* residual, void* out_bf16, float* out_f32,
                  int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups,
                  int cout, int cout_pad, int wgn, int splitk, void* scratch, size_t scratch_bytes, void* stream) {
    return op_conv3d_impl(xa, ca, xb, cb, w, bias, x1a, c1a, x1b, c1b, w1, bias2, temb, temb_stride, residual, out_bf16, out_f32, N, Din, Hin, Win,
                          ksize, stride, pad, ups, cout, cout_pad, wgn, splitk, scratch, scratch_bytes, stream, nullptr, nullptr);
}

/* The producer -> GroupNorm pair exactly as the inference plans launch it: a 3^3 stride-1 conv (bias only) whose epilogue - or whose
 * write-through split-K finalize - leaves the GroupNorm partial slabs of its bf16 output, then the ONE-launch GroupNorm(+SiLU)
 * (gn_fused_apply_kernel, write-through stores) that folds those slabs.  conv_out [M][round32(cout)] and gn_out (same shape) are bf16
 * NDHWC.  scratch: split-K slabs + statistics slabs (ldm_op_conv3d_gn_scratch_bytes).  Returns LDM_ERR_UNSUPPORTED where the plans
 * would not take the one-launch path (channels per group > 64, more than 512 slab rows per sample). */
size_t ldm_op_conv3d_gn_scratch_bytes(int N, int D, int H, int W, int cout_pad, int splitk) {
    const size_t M = (size_t)N * D * H * W;
    return (size_t)(splitk > 1 ? splitk : 0) * M * cout_pad * 4 + ((M + 31) / 32 + 64) * cout_pad * 2 * 4 + 1024;
}
int ldm_op_conv3d_gn(const void* x, int cin, const void* w, const float* bias, const float* gamma, const float* beta, int groups, float eps,
                     int silu, void* conv_out, void* gn_out, int N, int D, int H, int W, int cout, int cout_pad, int wgn, int splitk,
                     void* scratch, size_t scratch_bytes, void* stream) {
    if (!x || !w || !gamma || !beta || !conv_out || !gn_out || !scratch) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    const int C = rup(cout, 32);
    if (groups < 1 || C % groups || cout != C) return fail(LDM_ERR_BAD_ARG, "cout must be a multiple of 32 and of groups");
    if (scratch_bytes < ldm_op_conv3d_gn_scratch_bytes(N, D, H, W, cout_pad, splitk)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    const size_t M = (size_t)N * D * H * W;
    const size_t slab_bytes = (size_t)(splitk > 1 ? splitk : 0) * M * cout_pad * 4;
    float* stats = (float*)((char*)scratch + rup_sz(slab_bytes, 256));
    int nrb = 0;
    LDM_TRY(op_conv3d_impl(x, cin, nullptr, 0, w, bias, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, conv_out, nullptr,
                           N, D, H, W, 3, 1, 1, 0, cout, cout_pad, wgn, splitk, scratch, slab_bytes, stream, stats, &nrb));
    const int DHW = D * H * W;
    if (C / groups > 64 || nrb > 512) return fail(LDM_ERR_UNSUPPORTED, "the plans use the two-launch GroupNorm here (%d channels per group, %d slab rows)", C / groups, nrb);
    GnFusedParams g{}; g.xa = (const bf16_t*)conv_out; g.xb = nullptr; g.ca = C; g.cb = 0; g.sa = stats; g.sb = nullptr; g.nrb_a = nrb; g.nrb_b = 0;
    g.groups = groups; g.DHW = DHW; g.N = N; g.silu = silu; g.eps = eps; g.gamma = gamma; g.beta = beta; g.out = (bf16_t*)gn_out;
    const int chunks = gn_row_chunks(N, C, DHW, gn_fused_blocks(), 32, &g.rows_per_block);
    launch_gn_fused(g, chunks, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* The split-K conv -> GroupNorm pair as the inference plans launch it at the 12^3 / 6^3 levels (OP_CONV + OP_FIN_GN, csrc/fin_gn.h): a 3^3
 * stride-1 conv split over K (splitk >= 2) that writes its fp32 slabs planar (one plane per GroupNorm group), then ONE launch in which
 * every workgroup owns a whole (sample, group): it sums the slabs, applies bias / per-sample channel bias `temb` / `residual`, rounds to
 * bf16, reduces the group's statistics and writes GroupNorm(+SiLU) of the rounded tensor to gn_out; conv_out (optional) receives the
 * un-normalised bf16 tensor.  scratch: the split-K slabs (ldm_op_conv3d_fin_gn_scratch_bytes).
 * LDM_ERR_UNSUPPORTED where the plans keep the two launches (channels per group not a power of two in 4 ... 64, or more than 4096
 * (row, 4-channel) items per group). */
size_t ldm_op_conv3d_fin_gn_scratch_bytes(int N, int D, int H, int W, int cout_pad, int splitk) {
    return rup_sz((size_t)splitk * N * D * H * W * cout_pad * 4, 256);
}
int ldm_op_conv3d_fin_gn(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                         const float* gamma, const float* beta, int groups, float eps, int silu, void* conv_out, void* gn_out,
                         int N, int D, int H, int W, int cout, int cout_pad, int wgn, int splitk, void* scratch, size_t scratch_bytes,
                         void* stream) {
    if (!x || !w || !gamma || !beta || !gn_out || !scratch) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    const int C = rup(cout, 32);
    if (groups < 1 || C % groups || cout != C || splitk < 2) return fail(LDM_ERR_BAD_ARG, "cout must be a multiple of 32 and of groups, splitk >= 2");
    if (!fin_gn_ok(C, groups, D * H * W) || cout_pad % (C / groups))
        return fail(LDM_ERR_UNSUPPORTED, "the plans keep finalize and GroupNorm apart here (%d channels per group, %d rows)", C / groups, D * H * W);
    if (scratch_bytes < ldm_op_conv3d_fin_gn_scratch_bytes(N, D, H, W, cout_pad, splitk)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    const size_t slab_bytes = rup_sz((size_t)splitk * N * D * H * W * cout_pad * 4, 256);
    FinGnParams q{}; q.gamma = gamma; q.beta = beta; q.y = (bf16_t*)gn_out; q.groups = groups; q.silu = silu; q.eps = eps; q.lg = fin_gn_lg(C, groups);
    LDM_TRY(op_conv3d_impl(x, cin, nullptr, 0, w, bias, nullptr, 0, nullptr, 0, nullptr, nullptr, temb, temb_stride, residual, conv_out, nullptr,
                           N, D, H, W, 3, 1, 1, 0, cout, cout_pad, wgn, splitk, scratch, slab_bytes, stream, nullptr, nullptr, &q));
    return 0;
}

size_t ldm_op_group_norm_scratch_bytes(int N, int C, int DHW) {
    int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
    return ((size_t)N * nslab * C * 2 + (size_t)N * C * 2) * 4 + 512;
}

int ldm_op_group_norm(const void* xa, int ca, const void* xb, int cb, const float* gamma, const float* beta,
                      int groups, float eps, int silu, void* out, int N, int DHW, void* scratch, size_t scratch_bytes,
                      void* stream) {
    if (!xa || !gamma || !beta || !out || !scratch) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!xb) cb = 0;
    const int C = ca + cb;
    if (C % 8 || ca % 8 || groups < 1 || C % groups) return fail(LDM_ERR_BAD_ARG, "bad channel / group counts");
    if (scratch_bytes < ldm_op_group_norm_scratch_bytes(N, C, DHW)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    const int cvec = C / 8;
    int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
    float* partial = (float*)scratch;
    float* ab = partial + (size_t)N * nslab * C * 2;
    hipStream_t s = (hipStream_t)stream;
    GnStatsParams sp{}; sp.xa = (const bf16_t*)xa; sp.xb = (const bf16_t*)xb; sp.ca = ca; sp.cb = cb; sp.DHW = DHW; sp.nslab = nslab;
    sp.rows_per_slab = rps; sp.partial = partial;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(nslab, N), dim3(256), 0, s, sp);
    GnFinalizeParams fp{}; fp.partial = partial; fp.nslab = nslab; fp.C = C; fp.Creal = C; fp.groups = groups; fp.DHW = DHW; fp.eps = eps;
    fp.gamma = gamma; fp.beta = beta; fp.ab = ab;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, N), dim3(256), 0, s, fp);
    GnApplyParams ap{}; ap.xa = sp.xa; ap.xb = sp.xb; ap.ca = ca; ap.cb = cb; ap.DHW = DHW; ap.N = N; ap.silu = silu; ap.ab = ab; ap.out = (bf16_t*)out;
    hipLaunchKernelGGL(gn_apply_kernel, dim3(grid_for((long)N * DHW * cvec, 256, 2048)), dim3(256), 0, s, ap);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- PatchDiscriminator building blocks (stage-1 GAN tail): generic-kernel-size convs as im2col + the 1x1 GEMM kernels ---- */
}  // extern "C" (templates need C++ linkage)
template <class T>
static int op_im2col(const void* x, void* col, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, int kmul, void* stream) {
    if (!x || !col || N < 1 || C < 1 || C > Cs || k < 1 || stride < 1 || pad < 0 || Kp < k * k * k * C || Kp % kmul) return fail(LDM_ERR_BAD_ARG, "bad argument");
    const int Do = (D + 2 * pad - k) / stride + 1, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    if (Do < 1 || Ho < 1 || Wo < 1) return fail(LDM_ERR_BAD_ARG, "empty output");
    hipLaunchKernelGGL(im2col_generic_kernel<T>, dim3(grid_for((long)N * Do * Ho * Wo * Kp, 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)x, (T*)col, N, D, H, W, Cs, C, k, stride, pad, Do, Ho, Wo, Kp);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <class T>
static int op_col2im(const void* dcol, void* dx, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, int kmul, void* stream) {
    if (!dcol || !dx || N < 1 || C < 1 || C > Cs || k < 1 || stride < 1 || pad < 0 || Kp < k * k * k * C || Kp % kmul) return fail(LDM_ERR_BAD_ARG, "bad argument");
    const int Do = (D + 2 * pad - k) / stride + 1, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    if (Do < 1 || Ho < 1 || Wo < 1) return fail(LDM_ERR_BAD_ARG, "empty output");
    hipLaunchKernelGGL(col2im_generic_kernel<T>, dim3(grid_for((long)N * D * H * W * Cs, 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)dcol, (T*)dx, N, D, H, W, Cs, C, k, stride, pad, Do, Ho, Wo, Kp);
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" {
int ldm_op_im2col(const void* x, void* col, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream) {
    return op_im2col<bf16_t>(x, col, N, D, H, W, Cs, C, k, stride, pad, Kp, 32, stream);
}
int ldm_op_col2im(const void* dcol, void* dx, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream) {
    return op_col2im<bf16_t>(dcol, dx, N, D, H, W, Cs, C, k, stride, pad, Kp, 32, stream);
}
int ldm_op_leaky_relu(const void* x, void* y, int64_t n, float slope, void* stream) {
    if (!x || !y || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(leaky_relu_kernel<bf16_t>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, (long)n, slope);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_leaky_relu_bwd(const void* x, const void* dy, void* dx, int64_t n, float slope, void* stream) {
    if (!x || !dy || !dx || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(leaky_relu_bwd_kernel<bf16_t>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, (long)n, slope);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* fp32 NCDHW [N][C][DHW] <-> bf16 NDHWC [N][DHW][Cs] (channels zero-padded to Cs): the layout conversions the plans do internally */
int ldm_op_pack_ncdhw(const float* x, void* out, int N, int C, int Cs, int64_t DHW, void* stream) {
    if (!x || !out || N < 1 || C < 1 || C > Cs || DHW < 1 || DHW >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_pack2(x, C, nullptr, 0, out, N, Cs, (int)DHW, false, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_unpack_ndhwc(const void* act, float* out, int N, int C, int Cs, int64_t DHW, void* stream) {
    if (!act || !out || N < 1 || C < 1 || C > Cs || DHW < 1 || DHW >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(unpack_ndhwc_kernel<bf16_t>, dim3(grid_for((long)N * C * DHW)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)act, out, N, C, Cs, (int)DHW);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- the same building blocks on fp32 NDHWC tensors (the reference trains the PatchDiscriminator in fp32 when AMP is off,
 *      3d_ldm/train_autoencoder.py:150-158,454-494; `--precision fp32`): exact fp32 MFMA (csrc/f32_path.h, f32_train.h).
 *      Channels / K are multiples of 16, Cout padded to 64 weight rows. ------------------------------------------------------ */
int ldm_op_im2col_f32(const float* x, float* col, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream) {
    return op_im2col<float>(x, col, N, D, H, W, Cs, C, k, stride, pad, Kp, 16, stream);
}
int ldm_op_col2im_f32(const float* dcol, float* dx, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream) {
    return op_col2im<float>(dcol, dx, N, D, H, W, Cs, C, k, stride, pad, Kp, 16, stream);
}
int ldm_op_leaky_relu_f32(const float* x, float* y, int64_t n, float slope, void* stream) {
    if (!x || !y || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(leaky_relu_kernel<float>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, slope);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_leaky_relu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n, float slope, void* stream) {
    if (!x || !dy || !dx || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(leaky_relu_bwd_kernel<float>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, (long)n, slope);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_pack_ncdhw_f32(const float* x, float* out, int N, int C, int Cs, int64_t DHW, void* stream) {
    if (!x || !out || N < 1 || C < 1 || C > Cs || DHW < 1 || DHW >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_pack2(x, C, nullptr, 0, out, N, Cs, (int)DHW, true, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_unpack_ndhwc_f32(const float* act, float* out, int N, int C, int Cs, int64_t DHW, void* stream) {
    if (!act || !out || N < 1 || C < 1 || C > Cs || DHW < 1 || DHW >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(unpack_ndhwc_kernel<float>, dim3(grid_for((long)N * C * DHW)), dim3(256), 0, (hipStream_t)stream, act, out, N, C, Cs, (int)DHW);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* out[M][couts] = x[M][K] w[cout_pad][K]^T + bias (fp32, exact fp32 MFMA): K % 16 == 0, cout_pad % 64 == 0 weight rows (rows >= cout zero),
 * couts = stored output channels (% 4 == 0, >= cout; columns >= cout receive the products of the zero rows). */
int ldm_op_gemm_f32(const float* x, int K, const float* w, const float* bias, float* out, int64_t M, int cout, int cout_pad, int couts, void* stream) {
    if (!x || !w || !out || M < 1 || M >= (1L << 31) || K < 16 || K % 16 || cout < 1 || cout_pad % 64 || cout_pad < cout || couts % 4 || couts < cout || couts > cout_pad)
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    Conv32Params p{}; p.xa = x; p.ca = K; p.w = w; p.N = 1; p.Din = p.Dout = (int)M; p.Hin = p.Win = p.Hout = p.Wout = 1;
    p.ksize = 1; p.stride = 1; p.pad = 0; p.M = (int)M; p.CoutS = couts; p.CoutPad = cout_pad; p.CoutReal = cout;
    p.nchunk = K / 16; p.steps = p.nchunk; p.splitk = 1; p.steps_per_split = p.steps; p.mtiles = (int)((M + 127) / 128);
    p.bias = bias; p.out = out;
    const int bn = cout_pad % 128 == 0 ? 128 : 64;
    p.ntiles = cout_pad / bn;
    launch_conv32(p, false, bn, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* out[M][couts] = (xa | xb)[M][ca + cb] w[cout_pad][ca + cb]^T + bias (+ residual[M][couts]) on fp32 operands as three bf16 MFMAs per product
 * (gemm_light_x3.h: the 1x1x1 convolutions of the fp32 inference plans).  ca, cb % 32 == 0 (cb = 0: one source), cout_pad % 32 == 0,
 * couts % 32 == 0.  stats (optional): [ceil(M / rows)][couts][2] per-tile (sum, sum of squares) of the stored values, rows = 64 when
 * big else 32.  big: 64 x 64 tiles (cout_pad % 64 == 0) instead of 32 x 32; -1 = the planner's choice. */
int ldm_op_linear_f32x3(const float* xa, int ca, const float* xb, int cb, const float* w, const float* bias, const float* residual, float* out,
                        float* stats, int64_t M, int cout_pad, int couts, int big, void* stream) {
    if (!xa || !w || !out || M < 1 || ca < 32 || ca % 32 || cb < 0 || cb % 32 || (cb > 0 && !xb) || cout_pad < 32 || cout_pad % 32 || couts < 32 || couts % 32 ||
        couts > cout_pad || M * (int64_t)std::max(ca + cb, cout_pad) * 4 >= (1L << 31) || (big == 1 && cout_pad % 64))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    LightX3Params p{}; p.x = xa; p.xb = cb > 0 ? xb : nullptr; p.ca = ca; p.w = w; p.bias = bias; p.residual = residual; p.out = out; p.stats = stats;
    p.M = (int)M; p.K = ca + cb; p.CoutS = couts;
    HIP_TRY(launch_gemm_light_x3(p, cout_pad, big < 0 ? gemm_light_x3_big(M, cout_pad) : big, (hipStream_t)stream));
    return 0;
}
/* out[M][couts] = (xa | xb)[M][ca + cb] w[cout_pad][ca + cb]^T + bias (+ residual[M][couts]) on bf16 operands, fp32 accumulation, bf16 store:
 * the 1x1x1 convolutions of the bf16 plans as one operator call.  ca, cb % 32 == 0 (cb = 0: one source; K = ca + cb a multiple of 128, or
 * 32 / 64 / 96), cout_pad % 32 == 0, couts % 32 == 0.  stats (optional): [ceil(M / rows)][couts][2] per-tile (sum, sum of squares) of the
 * stored values, rows = 64 when big else 32.  big: 64-row tiles (cout_pad % 64 == 0); -1 = the planner's choice.
 * kernel: 0 = gemm_light_kernel (gemm_light.h), 1 = gemm_wg_kernel (gemm_wg.h: one source, K = 128 .. 512 in steps of 128, else
 * LDM_ERR_UNSUPPORTED), -1 = the planner's choice.  Both kernels give the same bits.
 * gn_slabs (optional): GroupNorm (gamma, beta [K], groups, eps; no activation) of xa in front of the GEMM, as the attention blocks run it:
 * xa is [M / gn_dhw samples][gn_dhw][K] and gn_slabs [samples * gn_nrb][K][2] the (sum, sum of squares) partial rows its producer left.
 * fold 0: gn_fused_apply_kernel into scratch ([M][K] bf16), then the GEMM (either kernel); fold 1: in gemm_wg_kernel's prologue (kernel 1 or
 * -1; LDM_ERR_UNSUPPORTED where the plans keep the two launches).  The residual is added as given (the plans pass the raw xa). */
int ldm_op_linear_bf16(const void* xa, int ca, const void* xb, int cb, const void* w, const float* bias, const void* residual, void* out,
                       float* stats, int64_t M, int cout_pad, int couts, int big, int kernel,
                       const float* gn_slabs, int gn_nrb, int gn_dhw, const float* gamma, const float* beta, int groups, float eps, int fold,
                       void* scratch, void* stream) {
    const int K = ca + (xb ? cb : 0);
    if (!xa || !w || !out || M < 1 || ca < 32 || ca % 32 || cb < 0 || cb % 32 || (cb > 0 && !xb) || cout_pad < 32 || cout_pad % 32 || couts < 32 || couts % 32 ||
        couts > cout_pad || M * (int64_t)std::max(K, cout_pad) * 2 >= (1L << 31) || (big == 1 && cout_pad % 64) || kernel < -1 || kernel > 1 ||
        !(K % 128 == 0 || K < 128) || K > 2048)
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    const bool one = !xb || cb == 0;
    const bool wg_shape = one && K % 128 == 0 && K >= 128 && K <= 512;
    if (kernel == 1 && !wg_shape) return fail(LDM_ERR_UNSUPPORTED, "gemm_wg_kernel takes one source and K = 128 .. 512 in steps of 128");
    LightParams p{}; p.x = (const bf16_t*)xa; p.xb = one ? nullptr : (const bf16_t*)xb; p.ca = one ? K : ca; p.w = (const bf16_t*)w; p.bias = bias;
    p.residual = (const bf16_t*)residual; p.out = (bf16_t*)out; p.stats = stats; p.M = (int)M; p.K = K; p.CoutS = couts;
    if (big < 0) big = cout_pad % 64 == 0 ? gemm_light_big(M, cout_pad) : 0;
    const int wg = kernel < 0 ? gemm_wg_ok(one, K, M) : kernel;
    if (gn_slabs) {
        if (!one || !gamma || !beta || groups < 1 || K % groups || K % 8 || K / groups > 64 || gn_nrb < 1 || gn_nrb > 512 || gn_dhw < 1 || M % gn_dhw || fold < 0 || fold > 1 ||
            (!fold && !scratch))
            return fail(LDM_ERR_BAD_ARG, "bad GroupNorm argument");
        if (fold) {
            if (!wg || !wg_shape || !gemm_wg_gn_shape_ok(K, gn_dhw, groups, gn_nrb, big))
                return fail(LDM_ERR_UNSUPPORTED, "the GroupNorm prologue needs gemm_wg_kernel, K >= 256, at most 16 slab rows, even groups of at most 64 channels");
            WgGnParams g{}; g.slabs = gn_slabs; g.gamma = gamma; g.beta = beta; g.nrb = gn_nrb; g.groups = groups; g.DHW = gn_dhw; g.eps = eps;
            HIP_TRY(launch_gemm_wg(p, cout_pad, big, (hipStream_t)stream, &g));
            return 0;
        }
        GnFusedParams g{}; g.xa = (const bf16_t*)xa; g.ca = K; g.sa = gn_slabs; g.nrb_a = gn_nrb; g.groups = groups; g.DHW = gn_dhw; g.N = (int)(M / gn_dhw);
        g.eps = eps; g.gamma = gamma; g.beta = beta; g.out = (bf16_t*)scratch;
        const int chunks = gn_row_chunks(g.N, K, gn_dhw, gn_fused_blocks(), 32, &g.rows_per_block);   // as Builder::gn_apply's one-launch form
        launch_gn_fused(g, chunks, (hipStream_t)stream);
        HIP_TRY(hipGetLastError());
        p.x = (const bf16_t*)scratch;
    }
    HIP_TRY(launch_gemm_1x1(p, cout_pad, big, wg, (hipStream_t)stream));
    return 0;
}
/* dw[ksplit][cout][K] = sum over the rows of dy[M][cdy]^T x[M][K] (partial matrices of `ksplit` row ranges; the caller sums them) */
int ldm_op_gemm_wgrad_f32(const float* dy, int cdy, const float* x, int K, float* dw, int cout, int64_t M, int ksplit, void* stream) {
    if (!dy || !x || !dw || M < 1 || M >= (1L << 31) || K < 4 || K % 4 || cdy % 4 || cout < 1 || cout > cdy || ksplit < 1 || ksplit > 64) return fail(LDM_ERR_BAD_ARG, "bad argument");
    Wgrad32Params q{}; q.dy = dy; q.cdy = cdy; q.x = x; q.cx = K; q.dw = dw; q.Cout = cout; q.Cin = K; q.dw_ld = K; q.dw_ci_off = 0;
    q.N = 1; q.Din = q.Dout = (int)M; q.Hin = q.Win = q.Hout = q.Wout = 1; q.ksize = 1; q.stride = 1; q.pad = 0; q.ups = 0; q.M = (int)M;
    q.co_tiles = (cout + 127) / 128; q.ci_tiles = (K + 127) / 128; q.ksplit = ksplit; q.slab_stride = (long)cout * K;
    launch_wgrad32(q, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
static bool head_dim_ok(int C, int d) { return (d == 32 || d == 64 || d == 128 || d == 256) && C >= d && C % d == 0; }
size_t ldm_op_group_norm_f32_scratch_bytes(int N, int C, int DHW, int groups) {
    int nslab = 1, rps = 1; gn_slabs(std::max(1, N), std::max(4, C), std::max(1, DHW), 4, 512, &nslab, &rps);
    return ((size_t)N * nslab * C * 2 * 2 + (size_t)N * C * 2 + (size_t)N * groups * 4 + (size_t)N * C * 2) * 4 + 1024;
}
/* y = act(GroupNorm(x)) on fp32 NDHWC [N][DHW][C] (act 0 none, 1 SiLU, 2 LeakyReLU(0.2)); C % 4 == 0, C <= 1024 */
int ldm_op_group_norm_f32(const float* x, int C, const float* gamma, const float* beta, int groups, float eps, int act, float* out,
                          int N, int DHW, void* scratch, size_t scratch_bytes, void* stream) {
    if (!x || !gamma || !beta || !out || !scratch || N < 1 || DHW < 1 || C < 4 || C % 4 || C > 1024 || groups < 1 || C % groups || act < 0 || act > 2)
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (scratch_bytes < ldm_op_group_norm_f32_scratch_bytes(N, C, DHW, groups)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    int nslab, rps; gn_slabs(N, C, DHW, 4, 512, &nslab, &rps);
    float* partial = (float*)scratch; float* ab = partial + (size_t)N * nslab * C * 2;
    hipStream_t s = (hipStream_t)stream;
    Gn32Params p{}; p.xa = x; p.ca = C; p.DHW = DHW; p.N = N; p.nslab = nslab; p.rows_per_slab = rps; p.silu = act; p.partial = partial; p.ab = ab; p.out = out;
    hipLaunchKernelGGL(gn_stats_f32_kernel, dim3(nslab, N), dim3(256), 0, s, p);
    GnFinalizeParams fp{}; fp.partial = partial; fp.nslab = nslab; fp.C = C; fp.Creal = C; fp.groups = groups; fp.DHW = DHW; fp.eps = eps;
    fp.gamma = gamma; fp.beta = beta; fp.ab = ab;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, N), dim3(256), 0, s, fp);
    hipLaunchKernelGGL(gn_apply_f32_kernel, dim3(grid_for((long)N * DHW * (C / 4), 256, 4096)), dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* backward of the above: dx (fp32), dgamma / dbeta (fp32 [C], summed over the batch); recomputes the forward statistics */
int ldm_op_group_norm_bwd_f32(const float* dy, const float* x, int C, const float* gamma, const float* beta, int groups, float eps, int act,
                              float* dx, float* dgamma, float* dbeta, int N, int DHW, void* scratch, size_t scratch_bytes, void* stream) {
    if (!dy || !x || !gamma || !beta || !dx || !dgamma || !dbeta || !scratch || N < 1 || DHW < 1 || C < 4 || C % 4 || C > 1024 || groups < 1 || C % groups)
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (scratch_bytes < ldm_op_group_norm_f32_scratch_bytes(N, C, DHW, groups)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    int nslab, rps; gn_slabs(N, C, DHW, 4, 512, &nslab, &rps);
    float* partial = (float*)scratch;                       // [N][nslab][C][2] (forward stats), then reused by the backward sums
    float* partial2 = partial + (size_t)N * nslab * C * 2;  // [N][nslab][C][2]
    float* ab = partial2 + (size_t)N * nslab * C * 2;       // [N][C][2]
    float* mr = ab + (size_t)N * C * 2;                     // [N][G][2]
    float* gsum = mr + (size_t)N * groups * 2;              // [N][G][2]
    float* dgn = gsum + (size_t)N * groups * 2;             // [N][C]
    float* dbn = dgn + (size_t)N * C;                       // [N][C]
    hipStream_t s = (hipStream_t)stream;
    Gn32Params p{}; p.xa = x; p.ca = C; p.DHW = DHW; p.N = N; p.nslab = nslab; p.rows_per_slab = rps; p.partial = partial;
    hipLaunchKernelGGL(gn_stats_f32_kernel, dim3(nslab, N), dim3(256), 0, s, p);
    GnFinalizeParams fp{}; fp.partial = partial; fp.nslab = nslab; fp.C = C; fp.Creal = C; fp.groups = groups; fp.DHW = DHW; fp.eps = eps;
    fp.gamma = gamma; fp.beta = beta; fp.ab = ab; fp.mr = mr;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, N), dim3(256), 0, s, fp);
    Gnb32Params q{}; q.dy = dy; q.xa = x; q.ca = C; q.ab = ab; q.mr = mr; q.gamma = gamma; q.groups = groups; q.DHW = DHW; q.N = N; q.silu = act;
    q.nslab = nslab; q.rows_per_slab = rps; q.partial = partial2; q.gsum = gsum; q.dxa = dx;
    GnBwdParams f{}; f.ca = C; f.cb = 0; f.gamma = gamma; f.groups = groups; f.DHW = DHW; f.N = N; f.nslab = nslab;
    f.partial = partial2; f.gsum = gsum; f.dgamma_n = N == 1 ? dgamma : dgn; f.dbeta_n = N == 1 ? dbeta : dbn;
    launch_gnb32(q, f, dgamma, dbeta, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- fp32-mode operator entries: the kernels of the fp32 plans, launched through the executor's own helpers (launch_conv32,
 * launch_fin32, launch_wgrad32, launch_gnb32, launch_attn_f32, launch_attn32_bwd), for per-kernel parity tests against fp64 */
int ldm_op_conv3d_f32_stats_blocks(int N, int dhwo, int couts, int* rows) {
    if (N < 1 || dhwo < 1 || couts < 4 || couts % 4 || couts > 1024 || !rows) return fail(LDM_ERR_BAD_ARG, "bad argument");
    return fin32_stats_blocks(N, dhwo, couts, rows);
}
int ldm_op_conv3d_f32(const float* xa, int ca, const float* xb, int cb, const float* w, const float* bias, const float* temb, int temb_stride,
                      const float* residual, float* out, int couts, float* out_ncdhw, float* stats, int N, int Din, int Hin, int Win,
                      int ksize, int stride, int pad, int ups, int cout, int cout_pad, int form, int bn, int splitk,
                      void* scratch, size_t scratch_bytes, void* stream) {
    if (!xa || !w || (!out == !out_ncdhw)) return fail(LDM_ERR_BAD_ARG, "null tensor argument (exactly one of out / out_ncdhw)");
    if (!xb) cb = 0;
    if (form != 0 && form != 1) return fail(LDM_ERR_BAD_ARG, "form 0 (fp32 MFMA) | 1 (3 x bf16)");
    const int kb = form ? 32 : 16;
    if (ca < kb || ca % kb || cb < 0 || cb % kb || cout < 1 || cout_pad % 64 || cout > cout_pad)
        return fail(LDM_ERR_BAD_ARG, "source channels must be multiples of %d, cout_pad of 64 (>= cout)", kb);
    if (out && (couts < cout || couts % 4 || couts > cout_pad)) return fail(LDM_ERR_BAD_ARG, "cout <= couts <= cout_pad, couts %% 4 == 0");
    if (out_ncdhw && (residual || stats)) return fail(LDM_ERR_BAD_ARG, "residual / stats need the NDHWC output");
    if (temb && temb_stride < cout_pad) return fail(LDM_ERR_BAD_ARG, "temb rows must hold cout_pad entries");
    if ((ksize != 1 && ksize != 3) || stride < 1 || stride > 2 || ups < 0 || ups > 2 || pad < 0 || pad > 2)
        return fail(LDM_ERR_UNSUPPORTED, "ksize 1|3, stride 1|2, pad 0..2, ups 0|1|2");
    if (bn != 0 && bn != 64 && bn != 128) return fail(LDM_ERR_BAD_ARG, "bn 0 (planner) | 64 | 128");
    if (splitk < 0 || splitk > 64) return fail(LDM_ERR_BAD_ARG, "splitk 0 (planner) .. 64");
    if (N < 1 || Din < 1 || Hin < 1 || Win < 1 || (long)N * Din * Hin * Win >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad input size");
    int exact = 0;
    if (ups == 2) { ups = 1; exact = 1; }            // zero insertion: the data gradient of a stride-2 conv
    const int Do = conv_out_size(Din, ksize, stride, pad, ups), Ho = conv_out_size(Hin, ksize, stride, pad, ups), Wo = conv_out_size(Win, ksize, stride, pad, ups);
    const long M = (long)N * Do * Ho * Wo;
    if (Do < 1 || Ho < 1 || Wo < 1 || M >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad output size");
    const int taps = ksize * ksize * ksize, nchunk = (ca + cb) / kb, steps = taps * nchunk;
    int pbn = 0, psk = 0;
    conv32_cfg(M, cout_pad, steps, form == 1, &pbn, &psk);
    if (!bn) bn = pbn;
    if (cout_pad % bn) return fail(LDM_ERR_BAD_ARG, "cout_pad %% bn != 0");
    int sk = splitk ? splitk : psk;
    { const int sps = (steps + sk - 1) / sk; sk = (steps + sps - 1) / sps; }     // as the planner normalises it
    if (sk > 1 && (!scratch || scratch_bytes < (size_t)sk * M * cout_pad * 4)) return fail(LDM_ERR_WORKSPACE, "scratch: splitk * M * cout_pad floats");
    if (stats && (sk < 2 || couts > 1024)) return fail(LDM_ERR_BAD_ARG, "stats come from the split-K finalize: splitk >= 2, couts <= 1024");
    Conv32Params p{};
    p.xa = xa; p.xb = cb ? xb : nullptr; p.ca = ca; p.cb = cb; p.w = w;
    p.N = N; p.Din = Din; p.Hin = Hin; p.Win = Win; p.Dout = Do; p.Hout = Ho; p.Wout = Wo;
    p.ksize = ksize; p.stride = stride; p.pad = pad; p.ups = ups; p.exact = exact; p.M = (int)M;
    p.CoutS = out ? couts : rup(cout, 32); p.CoutPad = cout_pad; p.CoutReal = cout;
    p.nchunk = nchunk; p.steps = steps; p.splitk = sk; p.steps_per_split = (steps + sk - 1) / sk;
    p.mtiles = (int)((M + 127) / 128); p.ntiles = cout_pad / bn;
    p.bias = bias; p.temb = temb; p.temb_stride = temb_stride; p.residual = residual; p.out = out; p.out_ncdhw = out_ncdhw;
    p.partial = sk > 1 ? (float*)scratch : nullptr;
    hipStream_t s = (hipStream_t)stream;
    launch_conv32(p, form == 1, bn, s);
    if (sk > 1) {
        if (stats) { p.stats = stats; p.stats_nrb = fin32_stats_blocks(N, Do * Ho * Wo, couts, &p.stats_rows); }
        launch_fin32(p, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
/* wt[tap'][ci][co] = w[taps-1-tap'][co][ci_off + ci] (fp32), the weights of the data-gradient conv of channels [ci_off, ci_off + ci_cnt)
 * of the input: w [taps][cout_pad][cin], wt [taps][round64(ci_cnt)][round32(cout)] (rows >= ci_cnt and columns >= cout zero).  desc_ws:
 * device memory for the launch's descriptor table (ldm_op_weight_flip_transpose_f32_ws_bytes). */
size_t ldm_op_weight_flip_transpose_f32_ws_bytes(int ksize, int cout, int ci_cnt) {
    const int taps = ksize * ksize * ksize;
    return 256 + (size_t)taps * ((rup(std::max(cout, 1), 32) + 63) / 64) * (rup(std::max(ci_cnt, 1), 64) / 64) * sizeof(int2);
}
int ldm_op_weight_flip_transpose_f32(const float* w, float* wt, int ksize, int cout, int cout_pad, int cin, int ci_off, int ci_cnt,
                                     void* desc_ws, size_t desc_ws_bytes, void* stream) {
    if (!w || !wt || !desc_ws || (ksize != 1 && ksize != 3) || cout < 1 || cout_pad < cout || cin < 1 || ci_off < 0 || ci_cnt < 1 || ci_off + ci_cnt > cin)
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (desc_ws_bytes < ldm_op_weight_flip_transpose_f32_ws_bytes(ksize, cout, ci_cnt)) return fail(LDM_ERR_WORKSPACE, "descriptor workspace too small");
    const int taps = ksize * ksize * ksize, rows = rup(ci_cnt, 64), cols = rup(cout, 32);
    WtDesc e{}; e.src_off = 0; e.dst_off = 0; e.taps = taps; e.cout = cout; e.cout_pad = cout_pad; e.cin = cin; e.rows = rows;
    e.ci_off = ci_off; e.ci_cnt = ci_cnt; e.col_tiles = (cols + 63) / 64; e.row_tiles = rows / 64;
    const int nb = e.col_tiles * e.row_tiles * taps;
    std::vector<int2> map(nb);
    for (int b = 0; b < nb; ++b) map[b] = make_int2(0, b);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)desc_ws;
    HIP_TRY(hipMemcpyAsync(ws, &e, sizeof(e), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + 256, map.data(), (size_t)nb * sizeof(int2), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                 // the host copies of the table die with this frame
    hipLaunchKernelGGL(weight_flip_transpose_batched_f32_kernel, dim3(nb), dim3(256), 0, s, (const WtDesc*)ws, (const int2*)(ws + 256),
                       (const char*)w, (char*)wt);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* dw[split][tap][co][dw_ci_off + ci] (fp32) = partial sums over the split's voxel range of dy[m][co] * x[src(m, tap)][ci] for co < cout,
 * ci < cin: dy [M][cdy], x [rows][cx] fp32 NDHWC (cdy, cx % 4 == 0); dw holds ksplit slabs of [k^3][cout][dw_ld] (dw_ci_off + cin <= dw_ld:
 * one source of a channel concatenation).  ksplit splits the 16-voxel steps; splits past the end leave zero slabs. */
int ldm_op_conv3d_wgrad_f32(const float* dy, int cdy, const float* x, int cx, float* dw, int cout, int cin, int dw_ld, int dw_ci_off,
                            int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups, int ksplit, void* stream) {
    if (!dy || !x || !dw) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (cdy < 4 || cdy % 4 || cx < 4 || cx % 4 || cout < 1 || cin < 1 || cout > cdy || cin > cx || dw_ci_off < 0 || dw_ci_off + cin > dw_ld)
        return fail(LDM_ERR_BAD_ARG, "bad channel counts");
    if ((ksize != 1 && ksize != 3) || stride < 1 || stride > 2 || ups < 0 || ups > 1 || pad < 0 || pad > 2) return fail(LDM_ERR_UNSUPPORTED, "ksize 1|3, stride 1|2, ups 0|1");
    if (ksplit < 1 || ksplit > 64) return fail(LDM_ERR_BAD_ARG, "ksplit must be in 1..64");
    if (N < 1 || Din < 1 || Hin < 1 || Win < 1 || (long)N * Din * Hin * Win >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad input size");
    const int Du = Din << ups, Hu = Hin << ups, Wu = Win << ups;
    const int pad_total = (stride == 2 && pad == 0 && ksize == 3) ? 1 : 2 * pad;
    const int Do = (Du + pad_total - ksize) / stride + 1, Ho = (Hu + pad_total - ksize) / stride + 1, Wo = (Wu + pad_total - ksize) / stride + 1;
    const long M = (long)N * Do * Ho * Wo;
    if (Do < 1 || Ho < 1 || Wo < 1 || M >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad output size");
    Wgrad32Params q{}; q.dy = dy; q.cdy = cdy; q.x = x; q.cx = cx; q.dw = dw; q.Cout = cout; q.Cin = cin; q.dw_ld = dw_ld; q.dw_ci_off = dw_ci_off;
    q.N = N; q.Din = Din; q.Hin = Hin; q.Win = Win; q.Dout = Do; q.Hout = Ho; q.Wout = Wo; q.ksize = ksize; q.stride = stride; q.pad = pad; q.ups = ups;
    q.M = (int)M; q.co_tiles = (cout + 127) / 128; q.ci_tiles = (cin + 127) / 128; q.ksplit = ksplit;
    q.slab_stride = (long)ksize * ksize * ksize * cout * dw_ld;
    launch_wgrad32(q, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* softmax(q k^T / sqrt(head_dim)) v on fp32 qkv [B*N][3C] -> out [B*N][C] (fp32); lse (optional) [B][C/head_dim][N]; x3 = 1: the 3 x bf16
 * products of the inference plans (head_dim 64, N >= 128; elsewhere the exact fp32 kernels run either way) */
int ldm_op_attention_f32(const float* qkv, float* out, float* lse, int B, int N, int C, int head_dim, int x3, void* stream) {
    if (!qkv || !out || B < 1 || N < 1 || (x3 != 0 && x3 != 1) || !head_dim_ok(C, head_dim) || (long)B * N * C * 3 >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument (head_dim 32|64|128|256, C % head_dim == 0)");
    Attn32Params p{}; p.qkv = qkv; p.out = out; p.B = B; p.N = N; p.C = C; p.heads = C / head_dim; p.d = head_dim;
    p.scale = 1.0f / sqrtf((float)head_dim); p.lse = lse; p.x3 = x3;
    HIP_TRY(launch_attn_f32(p, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
/* its backward: dqkv [B*N][3C] (fp32) from d_o [B*N][C], the forward's o and lse; delta_scratch: B * (C / head_dim) * N floats */
int ldm_op_attention_bwd_f32(const float* qkv, const float* o, const float* d_o, const float* lse, float* delta_scratch, float* dqkv,
                             int B, int N, int C, int head_dim, void* stream) {
    if (!qkv || !o || !d_o || !lse || !delta_scratch || !dqkv || B < 1 || N < 1 || !head_dim_ok(C, head_dim) || (long)B * N * C * 3 >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    Attn32BwdParams q{}; q.qkv = qkv; q.o = o; q.d_o = d_o; q.lse = lse; q.delta = delta_scratch; q.dqkv = dqkv;
    q.B = B; q.N = N; q.C = C; q.d = head_dim; q.heads = C / head_dim; q.scale = 1.0f / sqrtf((float)head_dim);
    HIP_TRY(launch_attn32_bwd(q, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
/* backward of y = act(GroupNorm(cat(xa, xb))) on fp32 NDHWC (act 0 none, 1 SiLU, 2 LeakyReLU(0.2)): dxa / dxb (+= acc_a / acc_b when
 * given), dgamma / dbeta summed over the batch; ca, cb % 4 == 0, ca + cb <= 1024; scratch from ldm_op_group_norm_f32_scratch_bytes */
int ldm_op_group_norm_bwd2_f32(const float* dy, const float* xa, int ca, const float* xb, int cb, const float* gamma, const float* beta,
                               int groups, float eps, int act, const float* acc_a, const float* acc_b, float* dxa, float* dxb,
                               float* dgamma, float* dbeta, int N, int DHW, void* scratch, size_t scratch_bytes, void* stream) {
    if (!xb) cb = 0;
    const int C = ca + cb;
    if (!dy || !xa || !gamma || !beta || !dxa || (cb && !dxb) || !dgamma || !dbeta || !scratch || N < 1 || DHW < 1 || ca < 4 || ca % 4 || cb < 0 ||
        cb % 4 || C > 1024 || groups < 1 || C % groups || act < 0 || act > 2 || (long)N * DHW * C >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (scratch_bytes < ldm_op_group_norm_f32_scratch_bytes(N, C, DHW, groups)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    int nslab, rps; gn_slabs(N, C, DHW, 4, 512, &nslab, &rps);
    float* partial = (float*)scratch;                       // [N][nslab][C][2] forward sums
    float* partial2 = partial + (size_t)N * nslab * C * 2;  // [N][nslab][C][2] backward sums
    float* ab = partial2 + (size_t)N * nslab * C * 2;       // [N][C][2]
    float* mr = ab + (size_t)N * C * 2;                     // [N][G][2]
    float* gsum = mr + (size_t)N * groups * 2;              // [N][G][2]
    float* dgn = gsum + (size_t)N * groups * 2;             // [N][C]
    float* dbn = dgn + (size_t)N * C;                       // [N][C]
    hipStream_t s = (hipStream_t)stream;
    Gn32Params p{}; p.xa = xa; p.xb = cb ? xb : nullptr; p.ca = ca; p.cb = cb; p.DHW = DHW; p.N = N; p.nslab = nslab; p.rows_per_slab = rps; p.partial = partial;
    hipLaunchKernelGGL(gn_stats_f32_kernel, dim3(nslab, N), dim3(256), 0, s, p);
    GnFinalizeParams fp{}; fp.partial = partial; fp.nslab = nslab; fp.C = C; fp.Creal = C; fp.groups = groups; fp.DHW = DHW; fp.eps = eps;
    fp.gamma = gamma; fp.beta = beta; fp.ab = ab; fp.mr = mr;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, N), dim3(256), 0, s, fp);
    Gnb32Params q{}; q.dy = dy; q.xa = xa; q.xb = p.xb; q.ca = ca; q.cb = cb; q.ab = ab; q.mr = mr; q.gamma = gamma; q.groups = groups; q.DHW = DHW;
    q.N = N; q.silu = act; q.nslab = nslab; q.rows_per_slab = rps; q.partial = partial2; q.gsum = gsum;
    q.acc_a = acc_a; q.acc_b = cb ? acc_b : nullptr; q.dxa = dxa; q.dxb = cb ? dxb : nullptr;
    GnBwdParams f{}; f.ca = ca; f.cb = cb; f.gamma = gamma; f.groups = groups; f.DHW = DHW; f.N = N; f.nslab = nslab;
    f.partial = partial2; f.gsum = gsum; f.dgamma_n = N == 1 ? dgamma : dgn; f.dbeta_n = N == 1 ? dbeta : dbn;
    launch_gnb32(q, f, dgamma, dbeta, s);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* adjoint of the nearest x2 upsample on fp32 NDHWC: dx[n][d][h][w][c] = sum of the 8 dy[n][2d + i][2h + j][2w + k][c]; C % 4 == 0,
 * D, H, W = the source (low-resolution) size */
int ldm_op_upsample_bwd_f32(const float* dy, float* dx, int N, int D, int H, int W, int C, void* stream) {
    if (!dy || !dx || N < 1 || D < 1 || H < 1 || W < 1 || C < 4 || C % 4) return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipLaunchKernelGGL(sumpool2_f32_kernel, dim3(grid_for((long)N * D * H * W * (C / 4), 256, 4096)), dim3(256), 0, (hipStream_t)stream, dy, dx, N, D, H, W, C);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t ldm_op_scale_intensity_percentiles_scratch_bytes(int B) { return (size_t)(B < 1 ? 1 : B) * (4 * 4096 * 4 + sizeof(PctState)) + 256; }
int ldm_op_scale_intensity_percentiles(const float* x, float* out, int B, int64_t n, float lower, float upper, float b_min, float b_max,
                                       void* scratch, size_t scratch_bytes, void* stream) {
    if (!x || !out || !scratch || B < 1 || n < 1 || n >= (1LL << 32) || lower < 0.f || upper > 100.f || lower > upper) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (scratch_bytes < ldm_op_scale_intensity_percentiles_scratch_bytes(B)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    hipStream_t s = (hipStream_t)stream;
    unsigned* hist = (unsigned*)scratch;
    PctState* st = (PctState*)((char*)scratch + (size_t)B * 4 * 4096 * 4);
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)B * 4 * 4096 * 4, s));
    hipLaunchKernelGGL(pct_init_kernel, dim3((B + 63) / 64), dim3(64), 0, s, st, B, (long)n, (double)lower, (double)upper);
    const int gx = grid_for(n, 256 * 16, 512);
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(pct_hist_kernel, dim3(gx, B), dim3(256), 0, s, x, (long)n, (const PctState*)st, hist, pass);
        hipLaunchKernelGGL(pct_scan_kernel, dim3(B), dim3(256), 0, s, st, hist, pass);
    }
    hipLaunchKernelGGL(pct_apply_kernel, dim3(grid_for(n, 256 * 4, 2048), B), dim3(256), 0, s, x, out, (long)n, (const PctState*)st, b_min, b_max);
    HIP_TRY(hipGetLastError());
    return 0;
}

static const char* metrics_check(int B, int C, int D, int H, int W, int win) {
    if (win < 3 || win > MT_MAXWIN || win % 2 == 0) return "win must be odd and in 3..11";
    if (B < 1 || C < 1 || D < 1 || H < 1 || W < 1) return "bad shape";
    if (D < win || H < win || W < win) return "every spatial extent must be at least win";
    if ((long)B * C * D * H * W >= (1L << 31)) return "volume pair too large";
    return nullptr;
}
size_t ldm_op_image_metrics_scratch_bytes(int B, int C, int D, int H, int W, int win) {
    if (metrics_check(B, C, D, H, W, win)) return 0;
    return (size_t)metrics_plan(B, C, D, H, W, win).groups * sizeof(MetricsPartial) + 256;
}
int ldm_op_image_metrics(const float* x, const int64_t* x_strides, const float* y, const int64_t* y_strides, int B, int C, int D, int H, int W,
                         const float* weights, int win, float data_range, float k1, float k2, float* out, float* ssim_map,
                         void* scratch, size_t scratch_bytes, void* stream) {
    if (!x || !y || !x_strides || !y_strides || !weights || !out || !scratch) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (const char* why = metrics_check(B, C, D, H, W, win)) return fail(LDM_ERR_BAD_ARG, "%s (win %d, volume %d x %d x %d)", why, win, D, H, W);
    if (x_strides[4] != 1 || y_strides[4] != 1) return fail(LDM_ERR_UNSUPPORTED, "W must be contiguous (stride 1): got %ld and %ld", (long)x_strides[4], (long)y_strides[4]);
    for (int i = 0; i < 4; ++i)
        if (x_strides[i] < 0 || y_strides[i] < 0) return fail(LDM_ERR_BAD_ARG, "negative stride");
    if (!(data_range > 0.f)) return fail(LDM_ERR_BAD_ARG, "data_range must be positive");
    const MetricsPlan m = metrics_plan(B, C, D, H, W, win);
    if (scratch_bytes < ldm_op_image_metrics_scratch_bytes(B, C, D, H, W, win)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    MetricsParams p{};
    p.x = x; p.y = y;
    for (int i = 0; i < 4; ++i) { p.xs[i] = (long)x_strides[i]; p.ys[i] = (long)y_strides[i]; }
    p.B = B; p.C = C; p.D = D; p.H = H; p.W = W; p.Do = D - win + 1; p.Ho = H - win + 1; p.Wo = W - win + 1;
    p.tiles_h = m.tiles_h; p.tiles_w = m.tiles_w; p.nchunk = m.nchunk; p.planes = m.planes;
    for (int i = 0; i < win; ++i) p.w[i] = weights[i];
    p.c1 = (k1 * data_range) * (k1 * data_range); p.c2 = (k2 * data_range) * (k2 * data_range);
    p.map = ssim_map; p.partial = (MetricsPartial*)scratch;
    hipStream_t s = (hipStream_t)stream;
    launch_image_metrics(p, win, m.groups, s);
    hipLaunchKernelGGL(metrics_finalize_kernel, dim3(B), dim3(MT_THREADS), 0, s, (const MetricsPartial*)scratch, (int)(m.groups / B),
                       (double)C * p.Do * p.Ho * p.Wo, (double)C * D * H * W, data_range, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Weights of the data-gradient conv: wt[tap'][ci][co] = w[taps-1-tap'][co][ci].  w: [taps][cout_pad][cin] bf16,
 * wt: [taps][round64(cin)][round32(cout)] bf16 (device memory, caller allocated). */
int ldm_op_weight_flip_transpose(const void* w, void* wt, int ksize, int cout, int cout_pad, int cin, void* stream) {
    if (!w || !wt || (ksize != 1 && ksize != 3) || cout < 1 || cin < 1 || cout_pad < cout) return fail(LDM_ERR_BAD_ARG, "bad argument");
    const int taps = ksize * ksize * ksize, rows = rup(cin, 64), cols = rup(cout, 32);
    hipLaunchKernelGGL(weight_flip_transpose_kernel, dim3((cols + 63) / 64, (rows + 63) / 64, taps), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)w, (bf16_t*)wt, taps, cout, cout_pad, cin, rows, 0, cin);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* dW[tap][co][ci] (fp32, [k^3][cout][cin]) of y = conv3d(x, w): dy [M][cdy] and x [rows][cx] are NDHWC bf16.
 * ksplit > 1 splits the voxel range: dw then holds ksplit partial matrices [ksplit][k^3][cout][cin] to be summed. */
int ldm_op_conv3d_wgrad(const void* dy, int cdy, const void* x, int cx, float* dw, int cout, int cin,
                        int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups, int ksplit, void* stream) {
    if (!dy || !x || !dw) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (cdy % 32 || cx % 32 || cout < 1 || cin < 1 || cout > cdy || cin > cx) return fail(LDM_ERR_BAD_ARG, "bad channel counts");
    if ((ksize != 1 && ksize != 3) || stride < 1 || stride > 2 || ups < 0 || ups > 1) return fail(LDM_ERR_UNSUPPORTED, "ksize 1|3, stride 1|2, ups 0|1");
    const int Du = Din << ups, Hu = Hin << ups, Wu = Win << ups;
    const int pad_total = (stride == 2 && pad == 0 && ksize == 3) ? 1 : 2 * pad;
    const int Do = (Du + pad_total - ksize) / stride + 1, Ho = (Hu + pad_total - ksize) / stride + 1, Wo = (Wu + pad_total - ksize) / stride + 1;
    const long M = (long)N * Do * Ho * Wo;
    if (M < 1 || M >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad output size");
    if ((long)M * cdy * 2 >= (1L << 32) || (long)N * Din * Hin * Win * cx * 2 >= (1L << 32)) return fail(LDM_ERR_UNSUPPORTED, "tensor exceeds 4 GiB");
    WgradParams p{}; p.dy = (const bf16_t*)dy; p.cdy = cdy; p.x = (const bf16_t*)x; p.cx = cx; p.dw = dw; p.Cout = cout; p.Cin = cin; p.dw_ld = cin; p.dw_ci_off = 0;
    p.N = N; p.Din = Din; p.Hin = Hin; p.Win = Win; p.Dout = Do; p.Hout = Ho; p.Wout = Wo; p.ksize = ksize; p.stride = stride; p.pad = pad; p.ups = ups;
    p.M = (int)M; p.co_tiles = (cout + 127) / 128; p.ci_tiles = (cin + 127) / 128;
    if (ksplit < 1 || ksplit > 64) return fail(LDM_ERR_BAD_ARG, "ksplit must be in 1..64");
    p.ksplit = ksplit; p.slab_stride = (long)ksize * ksize * ksize * cout * cin;
    LDM_TRY(launch_wgrad(p, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t ldm_op_group_norm_bwd_scratch_bytes(int N, int C, int DHW, int groups) {
    return ldm_op_group_norm_scratch_bytes(N, C, DHW) * 2 + ((size_t)N * groups * 4 + (size_t)N * C * 2) * 4 + 1024;
}

/* Backward of y = act(GroupNorm(cat(xa, xb))): dxa/dxb (bf16, += acc_a/acc_b when given), dgamma/dbeta (fp32 [C], summed
 * over the batch).  Recomputes the forward statistics (the training plan saves them instead). */
int ldm_op_group_norm_bwd(const void* dy, const void* xa, int ca, const void* xb, int cb, const float* gamma, const float* beta,
                          int groups, float eps, int silu, const void* acc_a, const void* acc_b, void* dxa, void* dxb,
                          float* dgamma, float* dbeta, int N, int DHW, void* scratch, size_t scratch_bytes, void* stream) {
    if (!dy || !xa || !gamma || !beta || !dxa || !dgamma || !dbeta || !scratch) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!xb) cb = 0;
    const int C = ca + cb;
    if (C % 8 || ca % 8 || groups < 1 || C % groups || (cb && !dxb)) return fail(LDM_ERR_BAD_ARG, "bad channel / group counts");
    if (scratch_bytes < ldm_op_group_norm_bwd_scratch_bytes(N, C, DHW, groups)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    const int cvec = C / 8;
    int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
    float* partial = (float*)scratch;                       // [N][nslab][C][2]
    float* ab = partial + (size_t)N * nslab * C * 2;        // [N][C][2]
    float* mr = ab + (size_t)N * C * 2;                     // [N][G][2]
    float* gsum = mr + (size_t)N * groups * 2;              // [N][G][2]
    float* dgn = gsum + (size_t)N * groups * 2;             // [N][C]
    float* dbn = dgn + (size_t)N * C;                       // [N][C]
    hipStream_t s = (hipStream_t)stream;
    GnStatsParams sp{}; sp.xa = (const bf16_t*)xa; sp.xb = (const bf16_t*)xb; sp.ca = ca; sp.cb = cb; sp.DHW = DHW; sp.nslab = nslab;
    sp.rows_per_slab = rps; sp.partial = partial;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(nslab, N), dim3(256), 0, s, sp);
    GnFinalizeParams fp{}; fp.partial = partial; fp.nslab = nslab; fp.C = C; fp.Creal = C; fp.groups = groups; fp.DHW = DHW; fp.eps = eps;
    fp.gamma = gamma; fp.beta = beta; fp.ab = ab; fp.mr = mr;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, N), dim3(256), 0, s, fp);
    GnBwdParams bp{}; bp.dy = (const bf16_t*)dy; bp.xa = sp.xa; bp.xb = sp.xb; bp.ca = ca; bp.cb = cb; bp.ab = ab; bp.mr = mr; bp.gamma = gamma;
    bp.groups = groups; bp.DHW = DHW; bp.N = N; bp.silu = silu; bp.nslab = nslab; bp.rows_per_slab = rps; bp.partial = partial; bp.gsum = gsum;
    bp.dgamma_n = dgn; bp.dbeta_n = dbn; bp.acc_a = (const bf16_t*)acc_a; bp.acc_b = (const bf16_t*)acc_b; bp.dxa = (bf16_t*)dxa; bp.dxb = (bf16_t*)dxb;
    hipLaunchKernelGGL(gn_bwd_stats_kernel, dim3(nslab, N), dim3(256), 0, s, bp);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(groups, N), dim3(256), 0, s, bp);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(grid_for((long)N * DHW * cvec, 256, 2048)), dim3(256), 0, s, bp);
    // parameter gradients: sum the per-sample rows (reuses the column-sum finalize with nslab = 1 layout [N][1][C][2]? no: plain loop)
    hipLaunchKernelGGL(rowsum_n_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)dgn, dgamma, N, C);
    hipLaunchKernelGGL(rowsum_n_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)dbn, dbeta, N, C);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- bf16 training-plan operator entries: the kernels of the bf16 backward plans, launched through the executor's own helpers
 * (launch_gnb, launch_colsum(_batched), launch_export(_batched), launch_wt_batched, launch_lin_dx / _dw, launch_sumpool2, launch_add_bf16,
 * launch_vae_heads(_bwd)) with the planner's geometry (gn_slabs, gnb_fold_chunks, lin_dx_nz), for per-kernel parity tests against fp64 */
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// descriptor tables of the batched entries: k descriptors at desc_ws, the block map at desc_ws + round256(k * sizeof(desc))
static size_t desc_ws_need(size_t desc_bytes, long nblocks) { return (desc_bytes + 255) / 256 * 256 + (size_t)nblocks * sizeof(int2); }
static int upload_descs(const void* d, size_t desc_bytes, const std::vector<int2>& map, void* ws, hipStream_t s) {
    char* w = (char*)ws;
    HIP_TRY(hipMemcpyAsync(w, d, desc_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w + (desc_bytes + 255) / 256 * 256, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                 // the host copies of the table die with this frame
    return 0;
}

size_t ldm_op_group_norm_bwd_saved_scratch_bytes(int N, int C, int DHW, int groups) {
    if (N < 1 || C < 8 || DHW < 1 || groups < 1) return 0;
    int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
    return ((size_t)N * nslab * C * 2 + (size_t)N * groups * 2 + (size_t)N * C * 2) * 4 + 256;
}
int ldm_op_group_norm_bwd_fold_chunks(int N, int C, int groups, int DHW) {
    if (N < 1 || C < 8 || C % 8 || groups < 1 || C % groups || DHW < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    int nslab, rps, rpb = 0; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
    const int chunks = gnb_fold_chunks(N, C, groups, DHW, nslab, &rpb);
    if (chunks < 1) return fail(LDM_ERR_UNSUPPORTED, "the fold form needs channels per group <= 64 (the plans use finalize + apply here)");
    return chunks;
}
/* Backward of y = act(GroupNorm(cat(xa, xb))) from the forward's saved ab [N][C][2] (u = a x + b) and mr [N][G][2] (mean, rstd), as the
 * training plans run it (OP_GNB): form 0 = stats + finalize + apply, 1 = stats + fold-apply (where Builder::backward_gn picks it, else
 * LDM_ERR_UNSUPPORTED).  cs (form 1, optional): per-row-chunk column sums of the stored dx, [N][chunks][ca][2] then [N][chunks][cb][2]. */
int ldm_op_group_norm_bwd_saved(const void* dy, const void* xa, int ca, const void* xb, int cb, const float* ab, const float* mr,
                                const float* gamma, int groups, int act, const void* acc_a, const void* acc_b, void* dxa, void* dxb,
                                float* dgamma, float* dbeta, float* cs, int N, int DHW, int form, void* scratch, size_t scratch_bytes,
                                void* stream) {
    if (!dy || !xa || !ab || !mr || !gamma || !dxa || !dgamma || !dbeta || !scratch) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!xb) cb = 0;
    const int C = ca + cb;
    if (ca < 8 || ca % 8 || cb < 0 || cb % 8 || groups < 1 || C % groups || (cb && !dxb)) return fail(LDM_ERR_BAD_ARG, "bad channel / group counts");
    if (act < 0 || act > 2 || (form != 0 && form != 1) || (cs && form != 1)) return fail(LDM_ERR_BAD_ARG, "act 0|1|2, form 0|1, cs needs form 1");
    if (N < 1 || DHW < 1 || (long)N * DHW * C >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad size");
    if (!aligned16(dy) || !aligned16(xa) || !aligned16(xb) || !aligned16(dxa) || !aligned16(dxb) || !aligned16(acc_a) || !aligned16(acc_b))
        return fail(LDM_ERR_BAD_ARG, "bf16 tensors must be 16-byte aligned");
    if (scratch_bytes < ldm_op_group_norm_bwd_saved_scratch_bytes(N, C, DHW, groups)) return fail(LDM_ERR_WORKSPACE, "scratch too small");
    int nslab, rps; gn_slabs(N, C, DHW, 8, 512, &nslab, &rps);
    int rpb = 0, chunks = 0;
    if (form == 1) {
        chunks = gnb_fold_chunks(N, C, groups, DHW, nslab, &rpb);
        if (chunks < 1) return fail(LDM_ERR_UNSUPPORTED, "the fold form needs channels per group <= 64");
    }
    float* partial = (float*)scratch;                       // [N][nslab][C][2]
    float* gsum = partial + (size_t)N * nslab * C * 2;      // [N][G][2]
    float* dgn = gsum + (size_t)N * groups * 2;             // [N][C]
    float* dbn = dgn + (size_t)N * C;                       // [N][C]
    GnBwdParams p{}; p.dy = (const bf16_t*)dy; p.xa = (const bf16_t*)xa; p.xb = cb ? (const bf16_t*)xb : nullptr; p.ca = ca; p.cb = cb;
    p.ab = ab; p.mr = mr; p.gamma = gamma; p.groups = groups; p.DHW = DHW; p.N = N; p.silu = act; p.nslab = nslab; p.rows_per_slab = rps;
    p.partial = partial; p.gsum = gsum; p.dgamma_n = N == 1 ? dgamma : dgn; p.dbeta_n = N == 1 ? dbeta : dbn;
    p.acc_a = (const bf16_t*)acc_a; p.acc_b = cb ? (const bf16_t*)acc_b : nullptr; p.dxa = (bf16_t*)dxa; p.dxb = cb ? (bf16_t*)dxb : nullptr;
    p.rows_per_block = rpb; p.cs = cs;
    launch_gnb(p, chunks, dgamma, dbeta, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Column-sum finalize (OP_COLSUM / OP_COLSUM_BATCH).  desc: k rows of {partial_off, out_off (floats into partial / out), N, nslab, C,
 * accumulate_over_n, count, out_stride}; partial [N][nslab][C][2] (the sums in the first of each pair).  batched 0: k == 1,
 * colsum_finalize_kernel; 1: one colsum_finalize_batched_kernel launch over every descriptor, its table built in desc_ws. */
static const int COLSUM_DESC = 8;
static bool colsum_desc_ok(const int64_t* d) {
    return d[0] >= 0 && d[1] >= 0 && d[2] >= 1 && d[3] >= 1 && d[4] >= 1 && (d[5] == 0 || d[5] == 1) && d[6] >= 1 && d[6] <= d[4] &&
           (d[5] == 1 || d[7] >= d[6]) && d[2] * d[3] * d[4] * 2 < (1L << 31) && d[2] * d[7] < (1L << 31);
}
size_t ldm_op_colsum_finalize_ws_bytes(const int64_t* desc, int k) {
    if (!desc || k < 1) return 0;
    long nb = 0;
    for (int j = 0; j < k; ++j) { const int64_t* d = desc + (size_t)j * COLSUM_DESC; nb += ((d[6] + 15) / 16) * (d[5] ? 1 : d[2]); }
    return desc_ws_need(k * sizeof(ColsumDesc), nb);
}
int ldm_op_colsum_finalize(const float* partial, float* out, const int64_t* desc, int k, int batched, void* desc_ws, size_t desc_ws_bytes,
                           void* stream) {
    if (!partial || !out || !desc || k < 1 || (batched != 0 && batched != 1) || (!batched && k != 1)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    for (int j = 0; j < k; ++j)
        if (!colsum_desc_ok(desc + (size_t)j * COLSUM_DESC)) return fail(LDM_ERR_BAD_ARG, "bad column-sum descriptor %d", j);
    hipStream_t s = (hipStream_t)stream;
    if (!batched) {
        const int64_t* d = desc;
        launch_colsum(partial + d[0], out + d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], (int)d[6], (int)d[7], s);
    } else {
        if (!desc_ws || desc_ws_bytes < ldm_op_colsum_finalize_ws_bytes(desc, k)) return fail(LDM_ERR_WORKSPACE, "descriptor workspace too small");
        char* base = (char*)partial;                      // one base for both sides: out as a signed byte offset from partial
        std::vector<ColsumDesc> ds; std::vector<int2> map;
        for (int j = 0; j < k; ++j) {
            const int64_t* d = desc + (size_t)j * COLSUM_DESC;
            ColsumDesc e{}; e.partial_off = (long)d[0] * 4; e.out_off = (long)((char*)(out + d[1]) - base);
            e.N = (int)d[2]; e.nslab = (int)d[3]; e.C = (int)d[4]; e.accumulate_over_n = (int)d[5]; e.count = (int)d[6]; e.out_stride = (int)d[7];
            e.gx = (e.count + 15) / 16;
            const int nb = e.gx * (e.accumulate_over_n ? 1 : e.N);
            for (int b = 0; b < nb; ++b) map.push_back(make_int2(j, b));
            ds.push_back(e);
        }
        LDM_TRY(upload_descs(ds.data(), ds.size() * sizeof(ds[0]), map, desc_ws, s));
        char* w = (char*)desc_ws;
        launch_colsum_batched((const ColsumDesc*)w, (const int2*)(w + (k * sizeof(ColsumDesc) + 255) / 256 * 256), (int)map.size(), base, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Weight-gradient export (OP_EXPORT / OP_EXPORT_BATCH): dst[dst_off + (co * cin + ci) * taps + t] = sum over nsplit slabs of
 * src[src_off + k * slab_stride + (t * rows_total + row_off + co) * ld + col_off + ci].  desc: k rows of {src_off, dst_off (floats),
 * slab_stride, taps (<= 27), rows_total, ld, row_off, col_off, cout, cin, nsplit}.  batched 0: k == 1, grad_export_kernel; 1: one
 * grad_export_batched_kernel launch, its table built in desc_ws. */
static const int EXPORT_DESC = 11;
static bool export_desc_ok(const int64_t* d) {
    return d[0] >= 0 && d[1] >= 0 && d[3] >= 1 && d[3] <= 27 && d[8] >= 1 && d[9] >= 1 && d[6] >= 0 && d[6] + d[8] <= d[4] &&
           d[7] >= 0 && d[7] + d[9] <= d[5] && d[10] >= 1 && d[10] <= 64 && (d[10] == 1 || d[2] >= d[3] * d[4] * d[5]) && d[8] < 65536;
}
size_t ldm_op_grad_export_ws_bytes(const int64_t* desc, int k) {
    if (!desc || k < 1) return 0;
    long nb = 0;
    for (int j = 0; j < k; ++j) { const int64_t* d = desc + (size_t)j * EXPORT_DESC; nb += ((d[9] + 63) / 64) * d[8]; }
    return desc_ws_need(k * sizeof(ExportDesc), nb);
}
int ldm_op_grad_export(const float* src, float* dst, const int64_t* desc, int k, int batched, void* desc_ws, size_t desc_ws_bytes, void* stream) {
    if (!src || !dst || !desc || k < 1 || (batched != 0 && batched != 1) || (!batched && k != 1)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    for (int j = 0; j < k; ++j)
        if (!export_desc_ok(desc + (size_t)j * EXPORT_DESC)) return fail(LDM_ERR_BAD_ARG, "bad export descriptor %d", j);
    hipStream_t s = (hipStream_t)stream;
    if (!batched) {
        const int64_t* d = desc;
        launch_export(src + d[0], dst + d[1], (int)d[3], (int)d[4], (int)d[5], (int)d[6], (int)d[7], (int)d[8], (int)d[9], (int)d[10], (long)d[2], s);
    } else {
        if (!desc_ws || desc_ws_bytes < ldm_op_grad_export_ws_bytes(desc, k)) return fail(LDM_ERR_WORKSPACE, "descriptor workspace too small");
        std::vector<ExportDesc> ds; std::vector<int2> map;
        for (int j = 0; j < k; ++j) {
            const int64_t* d = desc + (size_t)j * EXPORT_DESC;
            ExportDesc e{}; e.src_off = (long)d[0] * 4; e.dst_off = (long)d[1]; e.slab_stride = (long)d[2];
            e.taps = (int)d[3]; e.rows_total = (int)d[4]; e.ld = (int)d[5]; e.row_off = (int)d[6]; e.col_off = (int)d[7];
            e.cout = (int)d[8]; e.cin = (int)d[9]; e.nsplit = (int)d[10];
            const int nb = ((e.cin + 63) / 64) * e.cout;
            for (int b = 0; b < nb; ++b) map.push_back(make_int2(j, b));
            ds.push_back(e);
        }
        LDM_TRY(upload_descs(ds.data(), ds.size() * sizeof(ds[0]), map, desc_ws, s));
        char* w = (char*)desc_ws;
        launch_export_batched((const ExportDesc*)w, (const int2*)(w + (k * sizeof(ExportDesc) + 255) / 256 * 256), (int)map.size(),
                              (const char*)src, dst, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Every flipped / transposed bf16 weight of a backward plan in one launch (OP_WT_BATCH): for each of k rows {w_off, wt_off (bf16 elements),
 * ksize, cout, cout_pad, cin, ci_off, ci_cnt}: wt[wt_off + (tap' * round64(ci_cnt) + ci) * round32(cout) + co] =
 * w[w_off + ((taps-1-tap') * cout_pad + co) * cin + ci_off + ci], zero for ci >= ci_cnt or co >= cout. */
static const int WT_DESC = 8;
static bool wt_desc_ok(const int64_t* d) {
    return d[0] >= 0 && d[1] >= 0 && (d[2] == 1 || d[2] == 3) && d[3] >= 1 && d[4] >= d[3] && d[5] >= 1 && d[6] >= 0 && d[7] >= 1 &&
           d[6] + d[7] <= d[5] && d[4] * d[5] * 27 < (1L << 31);
}
static void wt_desc_geom(const int64_t* d, WtDesc& e) {
    const int taps = (int)(d[2] * d[2] * d[2]), rows = rup((int)d[7], 64), cols = rup((int)d[3], 32);
    e.src_off = (long)d[0] * 2; e.dst_off = (long)d[1] * 2; e.taps = taps; e.cout = (int)d[3]; e.cout_pad = (int)d[4]; e.cin = (int)d[5];
    e.rows = rows; e.ci_off = (int)d[6]; e.ci_cnt = (int)d[7]; e.col_tiles = (cols + 63) / 64; e.row_tiles = rows / 64;
}
size_t ldm_op_weight_flip_transpose_batched_ws_bytes(const int64_t* desc, int k) {
    if (!desc || k < 1) return 0;
    long nb = 0;
    for (int j = 0; j < k; ++j) { WtDesc e{}; wt_desc_geom(desc + (size_t)j * WT_DESC, e); nb += (long)e.col_tiles * e.row_tiles * e.taps; }
    return desc_ws_need(k * sizeof(WtDesc), nb);
}
int ldm_op_weight_flip_transpose_batched(const void* w, void* wt, const int64_t* desc, int k, void* desc_ws, size_t desc_ws_bytes, void* stream) {
    if (!w || !wt || !desc || k < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    for (int j = 0; j < k; ++j)
        if (!wt_desc_ok(desc + (size_t)j * WT_DESC)) return fail(LDM_ERR_BAD_ARG, "bad weight descriptor %d", j);
    if (!desc_ws || desc_ws_bytes < ldm_op_weight_flip_transpose_batched_ws_bytes(desc, k)) return fail(LDM_ERR_WORKSPACE, "descriptor workspace too small");
    std::vector<WtDesc> ds; std::vector<int2> map;
    for (int j = 0; j < k; ++j) {
        WtDesc e{}; wt_desc_geom(desc + (size_t)j * WT_DESC, e);
        const int nb = e.col_tiles * e.row_tiles * e.taps;
        for (int b = 0; b < nb; ++b) map.push_back(make_int2(j, b));
        ds.push_back(e);
    }
    hipStream_t s = (hipStream_t)stream;
    LDM_TRY(upload_descs(ds.data(), ds.size() * sizeof(ds[0]), map, desc_ws, s));
    char* ws = (char*)desc_ws;
    launch_wt_batched((const WtDesc*)ws, (const int2*)(ws + (k * sizeof(WtDesc) + 255) / 256 * 256), (int)map.size(), (const char*)w, (char*)wt, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Backward of y = W act(x) + b (act = SiLU on the input when silu_in) as OP_LIN_DX / OP_LIN_DW run it: dx[b][i] (row stride x_stride)
 * through ldm_op_linear_bwd_nz(O) output-row slices (part: nz * B * I floats) and their fold; dW [O][I], db [O] (optional).  W bf16 [O][I];
 * dy [B][dy_stride], x_pre [B][x_stride] fp32.  dx and dW may each be NULL (not both). */
int ldm_op_linear_bwd_nz(int O) { return O < 1 ? fail(LDM_ERR_BAD_ARG, "O < 1") : lin_dx_nz(O); }
int ldm_op_linear_bwd(const void* W, const float* dy, const float* x_pre, float* dx, float* dW, float* db, int B, int I, int O, int dy_stride,
                      int x_stride, int silu_in, float* part, size_t part_bytes, void* stream) {
    if (!dy || (!dx && !dW) || (db && !dW) || (dx && !W) || ((silu_in || dW) && !x_pre)) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || I < 1 || O < 1 || dy_stride < O || x_stride < I || (silu_in != 0 && silu_in != 1) || (long)O * I >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        const int nz = lin_dx_nz(O);
        if (!part || part_bytes < (size_t)nz * B * I * 4) return fail(LDM_ERR_WORKSPACE, "part: nz * B * I floats");
        launch_lin_dx((const bf16_t*)W, dy, x_pre, dx, part, B, I, O, dy_stride, x_stride, silu_in, nz, s);
    }
    if (dW) launch_lin_dw(dy, x_pre, dW, db, B, I, O, dy_stride, x_stride, silu_in, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* adjoint of the nearest x2 upsample on bf16 NDHWC (sumpool2_kernel): dx[n][d][h][w][c] = bf16(sum of the 8 fine dy); C % 8 == 0,
 * D, H, W = the source (low-resolution) size */
int ldm_op_upsample_bwd(const void* dy, void* dx, int N, int D, int H, int W, int C, void* stream) {
    if (!dy || !dx || N < 1 || D < 1 || H < 1 || W < 1 || C < 8 || C % 8 || (long)N * D * H * W * C * 8 >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (!aligned16(dy) || !aligned16(dx)) return fail(LDM_ERR_BAD_ARG, "bf16 tensors must be 16-byte aligned");
    launch_sumpool2((const bf16_t*)dy, (bf16_t*)dx, N, D, H, W, C, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* out = bf16(a + b) on n bf16 elements (n % 8 == 0) */
int ldm_op_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream) {
    if (!a || !b || !out || n < 8 || n % 8) return fail(LDM_ERR_BAD_ARG, "bad argument (n % 8 == 0)");
    if (!aligned16(a) || !aligned16(b) || !aligned16(out)) return fail(LDM_ERR_BAD_ARG, "bf16 tensors must be 16-byte aligned");
    launch_add_bf16((const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out, (long)(n / 8), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* AutoencoderKL sampling head (OP_VAE_HEADS): ml fp32 NCDHW [N][2L][DHW] (mu | log_var) -> mu, sigma = exp(0.5 clamp(lv, -30, 20)),
 * z = mu + sigma * eps (eps NULL: z = mu); every output optional */
int ldm_op_vae_heads(const float* ml, const float* eps, float* mu, float* sigma, float* z, int N, int L, int DHW, void* stream) {
    if (!ml || N < 1 || L < 1 || DHW < 1 || (long)N * 2 * L * DHW >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_vae_heads(ml, eps, mu, sigma, z, N, L, DHW, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* its backward (OP_VAE_HEADS_BWD): dy NDHWC [N*DHW][Cs] (Cs >= 2L; d_mu | d_lv | zero padding) from dz NDHWC [N*DHW][Ls] (Ls >= L), the
 * forward's ml and z (fp32 NCDHW [N][L][DHW]) and the optional KL-term gradients g_mu, g_sigma (fp32 NCDHW).  Storage of dz and dy:
 * bf16 (fp32 = 0) or fp32 (fp32 = 1, the fp32 precision mode). */
int ldm_op_vae_heads_bwd(const void* dz, int Ls, const float* ml, const float* z, const float* g_mu, const float* g_sigma, void* dy,
                         int N, int L, int Cs, int DHW, int fp32, void* stream) {
    if (!dz || !ml || !z || !dy) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (N < 1 || L < 1 || DHW < 1 || Ls < L || Cs < 2 * L || (fp32 != 0 && fp32 != 1) || (long)N * DHW * std::max(Cs, Ls) >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (fp32) launch_vae_heads_bwd<float>((const float*)dz, Ls, ml, z, g_mu, g_sigma, (float*)dy, N, L, Cs, DHW, s);
    else launch_vae_heads_bwd<bf16_t>((const bf16_t*)dz, Ls, ml, z, g_mu, g_sigma, (bf16_t*)dy, N, L, Cs, DHW, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* head_dim = 32 | 64 | 128 | 256 (C % head_dim == 0); lse may be NULL */
int ldm_op_attention_hd(const void* qkv, void* out, float* lse, int B, int N, int C, int head_dim, void* stream) {
    if (!qkv || !out || B < 1 || N < 1 || !head_dim_ok(C, head_dim)) return fail(LDM_ERR_BAD_ARG, "bad argument (head_dim 32|64|128|256, C % head_dim == 0)");
    AttnParams p{}; p.qkv = (const bf16_t*)qkv; p.out = (bf16_t*)out; p.B = B; p.N = N; p.C = C; p.d = head_dim; p.heads = C / head_dim;
    p.scale = 1.0f / sqrtf((float)head_dim); p.lse = lse;
    HIP_TRY(launch_attn_fwd(p, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_attention_bwd_hd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta_scratch, void* dqkv,
                            int B, int N, int C, int head_dim, void* stream) {
    if (!qkv || !o || !d_o || !lse || !delta_scratch || !dqkv || B < 1 || N < 1 || !head_dim_ok(C, head_dim)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    AttnBwdParams p{}; p.qkv = (const bf16_t*)qkv; p.o = (const bf16_t*)o; p.d_o = (const bf16_t*)d_o; p.lse = lse; p.delta = delta_scratch;
    p.dqkv = (bf16_t*)dqkv; p.B = B; p.N = N; p.C = C; p.d = head_dim; p.heads = C / head_dim; p.scale = 1.0f / sqrtf((float)head_dim);
    HIP_TRY(launch_attn_bwd(p, (hipStream_t)stream));
    return 0;
}
int ldm_op_attention(const void* qkv, void* out, int B, int N, int C, void* stream) {
    return ldm_op_attention_hd(qkv, out, nullptr, B, N, C, 64, stream);
}

/* attention forward that also saves the log-sum-exp rows, and its backward: dqkv [B*N][3C] from dO [B*N][C] (head_dim 64). */
int ldm_op_attention_train(const void* qkv, void* out, float* lse, int B, int N, int C, void* stream) {
    if (!lse) return fail(LDM_ERR_BAD_ARG, "bad argument");
    return ldm_op_attention_hd(qkv, out, lse, B, N, C, 64, stream);
}
int ldm_op_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta_scratch, void* dqkv,
                         int B, int N, int C, void* stream) {
    return ldm_op_attention_bwd_hd(qkv, o, d_o, lse, delta_scratch, dqkv, B, N, C, 64, stream);
}

// ---- RCCL (loaded lazily so the library itself has no hard dependency on librccl) -----------------------
typedef struct { char internal[128]; } rccl_uid;
typedef void* rccl_comm_t;
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(rccl_uid*) = nullptr;
    int (*CommInitRank)(rccl_comm_t*, int, rccl_uid, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
    int (*CommDestroy)(rccl_comm_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int*) = nullptr;
};
static RcclApi g_rccl;
static int rccl_load() {
    if (g_rccl.lib) return 0;
    // the copy the process has already loaded (torch links its own librccl) comes first: two different RCCL builds in one process
    // would each bring their own kernels and IPC state
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(LDM_ERR_RCCL, "cannot load librccl.so: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(rccl_uid*))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(rccl_comm_t*, int, rccl_uid, int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t))dlsym(h, "ncclAllReduce");
    g_rccl.Broadcast = (int (*)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t))dlsym(h, "ncclBroadcast");
    g_rccl.CommDestroy = (int (*)(rccl_comm_t))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    g_rccl.GetVersion = (int (*)(int*))dlsym(h, "ncclGetVersion");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.Broadcast || !g_rccl.CommDestroy)
        return fail(LDM_ERR_RCCL, "librccl.so lacks a required symbol");
    g_rccl.lib = h;
    return 0;
}
#define RCCL_TRY(x) do { int r_ = (x); if (r_ != 0) return fail(LDM_ERR_RCCL, "%s failed: %s", #x, \
    g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?"); } while (0)

struct ldm_comm { rccl_comm_t comm = nullptr; int rank = 0, world = 1; float* token = nullptr;
                  ldm_allreduce_fn fn = nullptr; void* user = nullptr;      // fn: caller-supplied transport (ldm_comm_init_custom)
                  int64_t n_allreduce = 0, bytes_allreduce = 0, n_broadcast = 0, bytes_broadcast = 0; };   // as handed to the transport

int ldm_comm_unique_id(char id[128]) {
    if (!id) return fail(LDM_ERR_BAD_ARG, "null id");
    LDM_TRY(rccl_load());
    rccl_uid u; RCCL_TRY(g_rccl.GetUniqueId(&u)); memcpy(id, u.internal, 128);
    return 0;
}
int ldm_comm_init(int rank, int world, const char id[128], ldm_comm** out) {
    if (!id || !out || world < 1 || rank < 0 || rank >= world) return fail(LDM_ERR_BAD_ARG, "bad argument");
    LDM_TRY(rccl_load());
    std::unique_ptr<ldm_comm> c(new ldm_comm()); c->rank = rank; c->world = world;
    rccl_uid u; memcpy(u.internal, id, 128);
    RCCL_TRY(g_rccl.CommInitRank(&c->comm, world, u, rank));
    HIP_TRY(hipMalloc((void**)&c->token, 256));
    HIP_TRY(hipMemset(c->token, 0, 256));
    HIP_TRY(hipDeviceSynchronize());
    *out = c.release();
    return 0;
}
/* A communicator whose all-reduce is the caller's function instead of RCCL: fn(user, buf, count, dtype, op, stream) must leave the
 * reduction over the `world` ranks in buf, ordered on `stream` (dtype / op as for ldm_comm_allreduce; non-zero return = failure).
 * Everything above the transport -- which ranges of the gradient buffer are handed over, when, on which stream, with which op, and
 * the join in front of the optimizer -- is the same code as with RCCL, so a test can stand in for the peers of a world > 1 job on one
 * GPU.  ldm_comm_broadcast is not available on such a communicator. */
int ldm_comm_init_custom(int rank, int world, ldm_allreduce_fn fn, void* user, ldm_comm** out) {
    if (!fn || !out || world < 1 || rank < 0 || rank >= world) return fail(LDM_ERR_BAD_ARG, "bad argument");
    std::unique_ptr<ldm_comm> c(new ldm_comm()); c->rank = rank; c->world = world; c->fn = fn; c->user = user;
    *out = c.release();
    return 0;
}
// ncclDataType: float32 = 7, bfloat16 = 9; ncclRedOp: sum = 0, avg = 4
int ldm_comm_allreduce(ldm_comm* c, void* buf, int64_t count, int dtype, int op, void* stream) {
    if (!c || !buf || count < 0 || dtype < 0 || dtype > 1 || op < 0 || op > 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    c->n_allreduce += 1; c->bytes_allreduce += count * (dtype == 0 ? 4 : 2);
    if (c->fn) {
        const int r = c->fn(c->user, buf, count, dtype, op, stream);
        return r ? fail(LDM_ERR_RCCL, "custom all-reduce returned %d", r) : 0;
    }
    RCCL_TRY(g_rccl.AllReduce(buf, buf, (size_t)count, dtype == 0 ? 7 : 9, op == 0 ? 0 : 4, c->comm, (hipStream_t)stream));
    return 0;
}
/* What this communicator has carried so far, counted where the bytes are handed to the transport (RCCL or the custom function):
 * out = {all-reduce calls, all-reduce bytes in the wire dtype, broadcast calls, broadcast bytes}. */
int ldm_comm_stats(const ldm_comm* c, int64_t out[4]) {
    if (!c || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    out[0] = c->n_allreduce; out[1] = c->bytes_allreduce; out[2] = c->n_broadcast; out[3] = c->bytes_broadcast;
    return 0;
}
/* 1 if the communicator's transport is RCCL (ncclAllReduce), 0 for a caller-supplied function */
int ldm_comm_is_rccl(const ldm_comm* c) { return c ? (c->fn ? 0 : 1) : -1; }
/* ncclGetVersion of the librccl this process uses (e.g. 22606), or a negative status when it cannot be loaded */
int ldm_comm_rccl_version(void) {
    LDM_TRY(rccl_load());
    int v = 0;
    if (!g_rccl.GetVersion) return fail(LDM_ERR_RCCL, "librccl.so lacks ncclGetVersion");
    RCCL_TRY(g_rccl.GetVersion(&v));
    return v;
}
int ldm_comm_broadcast(ldm_comm* c, void* buf, int64_t count, int dtype, int root, void* stream) {
    if (!c || !buf || count < 0 || dtype < 0 || dtype > 1 || root < 0 || root >= c->world) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (c->fn) return fail(LDM_ERR_UNSUPPORTED, "broadcast on a custom-transport communicator");
    c->n_broadcast += 1; c->bytes_broadcast += count * (dtype == 0 ? 4 : 2);
    RCCL_TRY(g_rccl.Broadcast(buf, buf, (size_t)count, dtype == 0 ? 7 : 9, root, c->comm, (hipStream_t)stream));
    return 0;
}
int ldm_comm_barrier(ldm_comm* c, void* stream) {
    if (!c) return fail(LDM_ERR_BAD_ARG, "null comm");
    if (c->fn) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return 0; }
    RCCL_TRY(g_rccl.AllReduce(c->token, c->token, 1, 7, 0, c->comm, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
void ldm_comm_destroy(ldm_comm* c) {
    if (!c) return;
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    if (c->token) (void)hipFree(c->token);
    delete c;
}
int ldm_comm_rank(const ldm_comm* c) { return c ? c->rank : -1; }
int ldm_comm_world(const ldm_comm* c) { return c ? c->world : -1; }

/* Attach (comm != NULL) or detach (NULL) the data-parallel gradient exchange of a model's training plans.  While attached,
 * ldm_unet_train_backward / ldm_vae_train_backward all-reduce (mean over ranks, fp32) the flat gradient buffer in buckets of
 * LDM_GRAD_BUCKET_MB (default 48) MB: a bucket's collective is queued on the communicator's own stream as soon as the backward pass
 * has finished that tail range of the buffer, overlapped with the rest of backward, and `stream` waits for the last one before the call's
 * work is complete in stream order.  Replaces DistributedDataParallel's bucketed hooks (3d_ldm/train_diffusion.py:147-149).
 * The communicator must outlive the attachment. */
int ldm_model_set_grad_sync(ldm_model* m, ldm_comm* comm) {
    if (!m) return fail(LDM_ERR_BAD_ARG, "null model");
    if (comm && !m->gsync.stream) HIP_TRY(hipStreamCreateWithFlags(&m->gsync.stream, hipStreamNonBlocking));
    m->gsync.comm = comm;
    return 0;
}
/* Wire format of the bucketed exchange: 0 = fp32 (default: what DistributedDataParallel reduces, 3d_ldm/train_diffusion.py:147-149),
 * 1 = bf16: on the communicator's stream every bucket is cast into a bf16 staging slice, all-reduced (avg) as bf16 and cast back into
 * the fp32 gradient buffer -- half the bytes per step for a ring that is xGMI-link bound (765 -> 382 MB for the benchmark UNet).
 * The staging slice (2 bytes per element of the largest bucket) is allocated at the first backward that needs it. */
int ldm_model_set_grad_wire(ldm_model* m, int dtype) {
    if (!m || dtype < 0 || dtype > 1) return fail(LDM_ERR_BAD_ARG, "wire dtype must be 0 (fp32) or 1 (bf16)");
    m->gsync.wire = dtype;
    return 0;
}
/* Buckets handed to the communicator's stream that no join has covered yet (0 = the exchange is quiescent: every collective of the
 * library's communicator is ordered in front of whatever the launch stream does next).  Host-side bookkeeping, no synchronisation. */
int ldm_model_grad_sync_pending(const ldm_model* m) { return m ? m->gsync.pending : -1; }
/* Timeline of the buckets of the LAST backward call (synchronises): issue_ms[k] = when bucket k was handed to the comm stream,
 * done_ms[k] = when its all-reduce finished, both relative to the start of that backward call; elems[k] = its size; then, at index
 * n (if max > n), the end of the backward call itself in issue_ms[n] (done_ms[n] = the same, elems[n] = 0).  Returns n. */
int ldm_model_grad_sync_trace(ldm_model* m, double* issue_ms, double* done_ms, int64_t* elems, int max) {
    if (!m || !issue_ms || !done_ms || !elems || max < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    GradSyncState& g = m->gsync;
    const int n = (int)g.elems.size();
    if (g.used < 2 + 2 * (size_t)n) return 0;
    HIP_TRY(hipEventSynchronize(g.ev[1]));
    for (int k = 0; k < n && k < max; ++k) {
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventSynchronize(g.ev[2 + 2 * k + 1]));
        HIP_TRY(hipEventElapsedTime(&a, g.ev[0], g.ev[2 + 2 * k])); HIP_TRY(hipEventElapsedTime(&b, g.ev[0], g.ev[2 + 2 * k + 1]));
        issue_ms[k] = a; done_ms[k] = b; elems[k] = g.elems[k];
    }
    if (max > n) { float e = 0.f; HIP_TRY(hipEventElapsedTime(&e, g.ev[0], g.ev[1])); issue_ms[n] = done_ms[n] = e; elems[n] = 0; }
    return n;
}

/* The gradient-exchange schedule of a training plan, readable without a GPU (plans are built on the host): one event per entry, in
 * launch order.  kind[k]: 0 = an op writes flat_grads[lo, lo + n) (final values), 1 = bucket: [lo, lo + n) is handed to the
 * communicator here, 2 = join (the launch stream waits for every bucket; the optimizer may follow), 3 = a write the dump does not
 * understand (a test failure).  op[k] = index of the launch-plan op.  Returns the number of events (may exceed max; only max are
 * written).  tests/test_grad_schedule_cpu.py checks: buckets tile [0, total) exactly once, no write into a range after its bucket
 * was issued, every element written before its bucket, join last. */
int ldm_model_grad_schedule(ldm_model* m, int B, int D, int H, int W, int* kind, int64_t* lo, int64_t* n, int* op, int max) {
    if (!m || max < 0 || (max > 0 && (!kind || !lo || !n || !op))) return fail(LDM_ERR_BAD_ARG, "bad argument");
    std::shared_ptr<Plan> p; LDM_TRY(get_plan(m, "train", B, D, H, W, &p));
    int cnt = 0;
    auto put = [&](int k, int64_t a, int64_t c, size_t oi) { if (cnt < max) { kind[cnt] = k; lo[cnt] = a; n[cnt] = c; op[cnt] = (int)oi; } ++cnt; };
    const ExportDesc* ed = (const ExportDesc*)p->exp_tab.h_descs.data(); const int2* em = (const int2*)p->exp_tab.h_map.data();
    for (size_t oi = p->bwd_begin; oi < p->ops.size(); ++oi) {
        const Op& o = p->ops[oi];
        switch (o.kind) {
            case OP_EXPORT_BATCH: {
                int last = -1;
                for (int b = o.rg.first; b < o.rg.end; ++b) if (em[b].x != last) {
                    last = em[b].x; const ExportDesc& e = ed[last];
                    put(0, e.dst_off, (int64_t)e.taps * e.cout * e.cin, oi);
                }
                break;
            }
            case OP_GNB: put(0, o.gn.dgamma_flat, o.gn.ca + o.gn.cb, oi); put(0, o.gn.dbeta_flat, o.gn.ca + o.gn.cb, oi); break;
            case OP_LIN_DW:
                if (o.lin.dW.base == BASE_IO4) put(0, (int64_t)(o.lin.dW.off / 4), (int64_t)o.lin.I * o.lin.O, oi);
                if (o.lin.db.base == BASE_IO4) put(0, (int64_t)(o.lin.db.off / 4), o.lin.O, oi);
                break;
            case OP_BUCKET: put(1, o.rg.first, o.rg.count, oi); break;
            case OP_BUCKET_JOIN: put(2, 0, 0, oi); break;
            default:
                for (const Ref* r : {&o.cv.out, &o.gn.out, &o.gn.dxa, &o.gn.dxb, &o.wg.dw,       // every ref a kernel writes (null unless the op is of that family)
                                     &o.lay.dst, &o.lay.a, &o.at.out, &o.at.lse, &o.at.delta, &o.at.dqkv, &o.lin.y, &o.lin.dx, &o.lin.dW, &o.lin.db, &o.lin.part,
                                     &o.el.out, &o.el.mu, &o.el.sigma, &o.el.z, &o.el.dy})
                    if (r->base == BASE_IO4) put(3, (int64_t)(r->off / 4), 0, oi);
        }
    }
    return cnt;
}

}  // extern "C"

// ---- gradient buckets (run_plan: OP_BUCKET / OP_BUCKET_JOIN) ----------------------------------------------------------------------
static hipEvent_t* gs_event(GradSyncState& g, size_t k) {
    while (g.ev.size() <= k) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; g.ev.push_back(e); }
    return &g.ev[k];
}
static int grad_sync_begin(GradSyncState& g, hipStream_t s) {
    // a previous backward that returned an error between a bucket and its join left buckets un-joined: this backward is ordered behind
    // them (the comm stream is in order: its last done-event covers all) and the bookkeeping starts clean
    if (g.pending > 0 && g.used > 2) HIP_TRY(hipStreamWaitEvent(s, g.ev[g.used - 1], 0));
    g.pending = 0;
    g.used = 2; g.elems.clear();                     // ev[0] = start of this backward, ev[1] = its end (recorded by the join)
    hipEvent_t* e0 = gs_event(g, 1); if (!e0) return fail(LDM_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(g.ev[0], s));
    return 0;
}
static int grad_sync_bucket(GradSyncState& g, float* buf, int64_t count, hipStream_t s) {
    if (!buf) return fail(LDM_ERR_BAD_ARG, "backward without a gradient buffer");
    if (!gs_event(g, g.used + 1)) return fail(LDM_ERR_HIP, "hipEventCreate failed");
    hipEvent_t issue = g.ev[g.used], done = g.ev[g.used + 1];
    HIP_TRY(hipEventRecord(issue, s));
    HIP_TRY(hipStreamWaitEvent(g.stream, issue, 0));
    if (g.wire == 1) {                                                                // bf16 on the wire: cast -> all-reduce(avg) -> cast back
        const size_t need = (size_t)count * 2;
        if (g.stage_bytes < need) {                                                   // first backward (or a larger bucket): grow once
            HIP_TRY(hipStreamSynchronize(g.stream));
            if (g.stage) (void)hipFree(g.stage);
            g.stage = nullptr; g.stage_bytes = 0;
            HIP_TRY(hipMalloc(&g.stage, rup_sz(need, 256)));
            g.stage_bytes = rup_sz(need, 256);
        }
        const int nb = grid_for((count + 7) / 8, 256, 2048);
        hipLaunchKernelGGL(grad_wire_pack_kernel, dim3(nb), dim3(256), 0, g.stream, (const float*)buf, (bf16_t*)g.stage, (long)count);
        LDM_TRY(ldm_comm_allreduce(g.comm, g.stage, count, 1, 1, g.stream));
        hipLaunchKernelGGL(grad_wire_unpack_kernel, dim3(nb), dim3(256), 0, g.stream, (const bf16_t*)g.stage, buf, (long)count);
        HIP_TRY(hipGetLastError());
    } else
        LDM_TRY(ldm_comm_allreduce(g.comm, buf, count, 0, 1, g.stream));             // fp32, mean over ranks
    HIP_TRY(hipEventRecord(done, g.stream));
    g.used += 2; g.elems.push_back(count); g.pending += 1;
    return 0;
}
static int grad_sync_join(GradSyncState& g, hipStream_t s) {
    if (g.used > 2) HIP_TRY(hipStreamWaitEvent(s, g.ev[g.used - 1], 0));             // the comm stream is in order: the last bucket covers all
    HIP_TRY(hipEventRecord(g.ev[1], s));
    g.pending = 0;
    return 0;
}
// a backward that exchanges nothing (a micro-batch in front of the last of its accumulation window): ordered behind stray buckets as
// grad_sync_begin orders itself, and the timeline of the "last backward" is empty (ldm_model_grad_sync_trace returns 0)
static int grad_sync_idle(GradSyncState& g, hipStream_t s) {
    if (g.pending > 0 && g.used > 2) HIP_TRY(hipStreamWaitEvent(s, g.ev[g.used - 1], 0));
    g.pending = 0;
    g.used = 0; g.elems.clear();
    return 0;
}
static int backward_lanes(ldm_model* m, hipStream_t s, LaneCtx* lanes) {
    const GradAccumState& a = m->gaccum;
    if (a.acc) { lanes->acc = a.acc; lanes->acc_assign = a.micro == 0; lanes->acc_scale = (float)(1.0 / a.count); }
    if (!m->gsync.comm) return 0;
    if (a.acc && a.micro < a.count - 1) return grad_sync_idle(m->gsync, s);
    lanes->sync = &m->gsync;
    return grad_sync_begin(m->gsync, s);
}

// ---- classifier-free guidance (concat conditioning; norm_elem.h) ------------------------------------------------------------------
// Every launch of the guided kernels sits here, behind the last launch of every older kernel: hipcc emits template kernels in the order
// of their first instantiation, so the code object keeps the layout it had (DESIGN.md section 3.7a').
static void guided_layout_launch(OpKind kind, const LayoutRec& l, const float* x, int cx, const float* cond, int cc, float fill, void* dst, hipStream_t s) {
    const int B = l.N / 2;
    const long total = (long)l.N * l.DHW * l.c_stored;
    if (kind == OP_PACK)
        hipLaunchKernelGGL((guided_pack2_ncdhw_kernel<bf16_t>), dim3(grid_for(total)), dim3(256), 0, s, x, cx, cond, cc, fill, (bf16_t*)dst, l.N, B, l.c_stored, l.DHW);
    else if (kind == OP_PACK32)
        hipLaunchKernelGGL((guided_pack2_ncdhw_kernel<float>), dim3(grid_for(total)), dim3(256), 0, s, x, cx, cond, cc, fill, (float*)dst, l.N, B, l.c_stored, l.DHW);
    else
        hipLaunchKernelGGL(guided_pack_im2col_kernel<>, dim3(grid_for((long)l.N * l.D * l.H * l.W * (l.c_stored / 8), 256, 16384)), dim3(256), 0, s, x, cx,
                           cond, cc, fill, (bf16_t*)dst, l.N, B, l.D, l.H, l.W, l.c_stored);
}
static void guided_combine_launch(const float* u, const float* c, float w, float* out, int64_t n, hipStream_t s) {
    if (n < 1) return;
    const int vec = (((uintptr_t)u | (uintptr_t)c | (uintptr_t)out) & 15) == 0;
    hipLaunchKernelGGL(guided_output_kernel<>, dim3(grid_for((n + 3) / 4, 256, 1024)), dim3(256), 0, s, u, c, w, out, (long)n, vec);
}
// Philox4x32-10 on the host: philox4x32_10 of norm_elem.h word for word, the high halves through 64-bit products
static void philox4x32_10_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
#define COND_DROP_STREAM 4u                          // beside the latent batch's streams 0 .. 2 and the rectified-flow timestep draw (3)

extern "C" {

/* out[i] = u[i] + w (c[i] - u[i]) over n fp32 elements (guidance_combine: the difference rounded once, then one fused multiply-add):
 * what MONAI's sampler hands its scheduler under classifier-free guidance, u the unconditional and c the conditional model output.
 * out may alias u. */
int ldm_guidance_combine(const float* u, const float* c, float w, float* out, int64_t n, void* stream) {
    if (!u || !c || !out || n < 0) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (out == c) return fail(LDM_ERR_BAD_ARG, "out may alias u, not c");
    guided_combine_launch(u, c, w, out, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Workspace of the guided entries for B samples (ldm_unet_denoise_step_guided) or chunks of B windows
 * (ldm_unet_denoise_step_windows_guided) of D x H x W: the guided plan at batch 2 B, then room for one doubled output [2 B][out][DHW],
 * which only the windowed entry uses. */
size_t ldm_unet_guided_workspace_bytes(ldm_model* m, int B, int D, int H, int W) {
    if (!m || m->type != 0) { fail(LDM_ERR_BAD_ARG, "not a UNet handle"); return 0; }
    if (B < 1 || B > (1 << 20)) { fail(LDM_ERR_BAD_ARG, "bad batch size"); return 0; }
    std::shared_ptr<Plan> p; if (get_plan(m, "unet_cfg", 2 * B, D, H, W, &p)) return 0;
    return rup_sz(p->ws_bytes, 256) + (size_t)2 * B * m->ucfg.out_channels * D * H * W * 4;
}

/* One whole denoising step under classifier-free guidance, from the caller's B-sample x and cond: the guided plan at batch 2 B
 * (samples 0 .. B-1: (x | fill), samples B .. 2B-1: (x | cond), MONAI's order) into eps_scratch [2 B][out][DHW], the combine
 * u + w (c - u) in place on its first half, then ldm_sampler_step on that half (n = B out DHW: the multistep state of a PNDM sampler is
 * that of B samples and holds guided outputs).  tbuf has 2 B entries; the sampler publishes the next t to all of them.  Every sampler
 * kind is taken.  cond NULL or cond_channels 0: LDM_ERR_BAD_ARG, nothing launched.  Graph mode: the whole step is ONE graph launch, and
 * w and fill are part of the replay key. */
int ldm_unet_denoise_step_guided(ldm_model* m, ldm_sampler* sp, float* x, int x_channels, const float* cond, int cond_channels,
                                 float w, float fill, float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!sp) return fail(LDM_ERR_BAD_ARG, "null sampler");
    if (!cond || cond_channels < 1) return fail(LDM_ERR_BAD_ARG, "classifier-free guidance needs a condition tensor (concat conditioning)");
    if (B < 1 || B > (1 << 20)) return fail(LDM_ERR_BAD_ARG, "bad batch size");
    if (m && m->type == 0 && x_channels != m->ucfg.out_channels) return fail(LDM_ERR_BAD_ARG, "x must have the UNet's out_channels (%d)", m->ucfg.out_channels);
    LDM_TRY(sampler_check_state(sp, (int64_t)B * x_channels * D * H * W));      // before the plan is built or anything is launched
    LDM_TRY(repaint_check(sp, (int64_t)B * x_channels * D * H * W, B));
    const Guide g{w, fill};
    return unet_step(m, {x, x_channels, cond, cond_channels, tbuf, eps_scratch, B, B, D, H, W, workspace, workspace_bytes, stream, sp, x, &g});
}

/* ldm_unet_denoise_step_windows under classifier-free guidance: each chunk of nb windows runs the guided plan at 2 nb from xw / cond_w,
 * its doubled output lands behind the plan's workspace (ldm_unet_guided_workspace_bytes(m, chunk, roi) counts it) and the combine writes
 * eps_w window by window; the blend-step kernels then run unchanged.  tbuf: at least 2 chunk entries.  Graph mode: ONE graph launch. */
int ldm_unet_denoise_step_windows_guided(ldm_model* m, ldm_sampler* sp, const ldm_window_grid* grid, float* x, int x_channels,
                                         const float* cond_w, int cond_channels, float w, float fill, float* xw, float* eps_w, float* tbuf,
                                         int chunk, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cond_w || cond_channels < 1) return fail(LDM_ERR_BAD_ARG, "classifier-free guidance needs a condition tensor (concat conditioning)");
    const Guide g{w, fill};
    return denoise_step_windows(m, sp, grid, x, x_channels, cond_w, cond_channels, xw, eps_w, tbuf, chunk, workspace, workspace_bytes, stream, &g);
}

/* Condition dropout of a training batch: slot b of cond [B][per_sample] (device) is overwritten with `fill` where the decision says so.
 * mask_in (HOST, [B], non-zero = drop) wins if given; otherwise slot b drops iff u < p with
 *   Philox4x32-10(counter = (0, idx[b], step, 0x1a7e0000 + 4), key = seed),  u = (word 0 >> 8) 2^-24,
 * a fifth stream in ldm_latent_batch's key layout: a function of (seed, step, dataset index) alone, never of the slot or of B.  idx is a
 * HOST array (NULL: 0 .. B-1).  The decisions are made on the host and reach the kernel by value; mask_out_host (optional, [B]) receives
 * them.  p = 0 drops nothing, p = 1 everything; nothing is launched when no slot drops.  Refused like ldm_latent_batch: B outside
 * 1 .. 64, p outside [0, 1], NULL cond, a negative index. */
int ldm_cond_dropout(float* cond, int B, int64_t per_sample, const int* idx, float p, float fill, const unsigned char* mask_in,
                     uint64_t seed, uint32_t step, unsigned char* mask_out_host, void* stream) {
    if (!cond) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || B > LATENT_BATCH_MAX) return fail(LDM_ERR_BAD_ARG, "batch size %d outside 1 .. %d", B, LATENT_BATCH_MAX);
    if (per_sample < 1 || per_sample > ((int64_t)1 << 33)) return fail(LDM_ERR_BAD_ARG, "bad sample size %lld", (long long)per_sample);
    if (!(p >= 0.f && p <= 1.f)) return fail(LDM_ERR_BAD_ARG, "drop probability %g outside [0, 1]", (double)p);
    if (idx) for (int b = 0; b < B; ++b) if (idx[b] < 0) return fail(LDM_ERR_BAD_ARG, "idx[%d] = %d is negative", b, idx[b]);
    unsigned long long mask = 0;
    for (int b = 0; b < B; ++b) {
        bool drop;
        if (mask_in) drop = mask_in[b] != 0;
        else {
            uint32_t r[4];
            philox4x32_10_host(0u, (uint32_t)(idx ? idx[b] : b), step, LATENT_STREAM_TAG + COND_DROP_STREAM, (uint32_t)seed, (uint32_t)(seed >> 32), r);
            drop = (float)(r[0] >> 8) * (1.0f / 16777216.0f) < p;
        }
        if (drop) mask |= 1ull << b;
        if (mask_out_host) mask_out_host[b] = drop ? 1 : 0;
    }
    if (!mask) return 0;
    const int vec = per_sample % 4 == 0 && ((uintptr_t)cond & 15) == 0;
    hipLaunchKernelGGL(cond_dropout_kernel<>, dim3(grid_for((per_sample + 3) / 4 * B, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       cond, (long)per_sample, B, mask, fill, vec);
    HIP_TRY(hipGetLastError());
    return 0;
}


// ---- ensemble statistics (ensemble.h): a running per-voxel (mean, m2) over member volumes, and the maps / scalars read off it ----
static bool ens_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 4, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 4;
    return a0 < b1 && b0 < a1;
}
static int ens_vec(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs) if ((uintptr_t)q % 16) return 0;
    return 1;
}
/* Folds members[b][0..n), b = 0 .. B-1 (fp32 device, member b at members + b * member_stride), into the state (mean, m2) that already
 * holds `count` members; the caller keeps the count.  count == 0: the state's contents are ignored. */
int ldm_ensemble_update(const float* members, int B, int64_t member_stride, int64_t n, float* mean, float* m2, int count, void* stream) {
    if (!members || !mean || !m2) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (B < 1 || n < 1 || count < 0) return fail(LDM_ERR_BAD_ARG, "B = %d, n = %lld, count = %d: B and n must be positive, count >= 0", B, (long long)n, count);
    if (count > 0x7fffffff - B) return fail(LDM_ERR_BAD_ARG, "count + B = %d + %d does not fit an int", count, B);
    if (member_stride < n) return fail(LDM_ERR_BAD_ARG, "member_stride %lld < n %lld", (long long)member_stride, (long long)n);
    const int64_t span = (int64_t)(B - 1) * member_stride + n;
    if (ens_overlap(members, span, mean, n) || ens_overlap(members, span, m2, n) || ens_overlap(mean, n, m2, n))
        return fail(LDM_ERR_BAD_ARG, "the members, mean and m2 ranges must not overlap");
    const int vec = ens_vec({members, mean, m2}) && member_stride % 4 == 0;
    hipLaunchKernelGGL(ensemble_update_kernel<>, dim3(grid_for((n + 3) / 4, 256, 1024)), dim3(ENS_THREADS), 0, (hipStream_t)stream, members, B,
                       (long)member_stride, (long)n, mean, m2, count, vec);
    HIP_TRY(hipGetLastError());
    return 0;
}
size_t ldm_ensemble_stats_scratch_bytes(int64_t n) {
    if (n < 1) { fail(LDM_ERR_BAD_ARG, "n must be positive, got %lld", (long long)n); return 0; }
    return (size_t)ens_blocks((long)n) * sizeof(EnsPartial);
}
/* std_out[i] (optional) = sqrt(max(m2[i], 0) / (count - ddof)); stats (device, LDM_ENS_STATS floats) = {mean std, max std, mean var,
 * mean (mean - target)^2 or 0 without a target, 0, 0, 0, 0}.  Two launches, fixed-order double partials in `scratch`. */
int ldm_ensemble_finalize(const float* mean, const float* m2, int count, int ddof, const float* target, float* std_out, float* stats,
                          void* scratch, size_t scratch_bytes, int64_t n, void* stream) {
    static_assert(ENS_STATS == LDM_ENS_STATS, "stats length of the header");
    if (!mean || !m2 || !stats || !scratch) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (n < 1) return fail(LDM_ERR_BAD_ARG, "n must be positive, got %lld", (long long)n);
    if (ddof != 0 && ddof != 1) return fail(LDM_ERR_BAD_ARG, "ddof must be 0 or 1, got %d", ddof);
    if (count < 0 || count - ddof < 1) return fail(LDM_ERR_BAD_ARG, "count - ddof = %d - %d < 1: not enough members", count, ddof);
    if ((uintptr_t)scratch % 8) return fail(LDM_ERR_BAD_ARG, "scratch not aligned to 8 bytes");
    const int nb = ens_blocks((long)n);
    if (scratch_bytes < (size_t)nb * sizeof(EnsPartial)) return fail(LDM_ERR_BAD_ARG, "scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)nb * sizeof(EnsPartial));
    if (std_out && (ens_overlap(std_out, n, mean, n) || ens_overlap(std_out, n, m2, n) || (target && ens_overlap(std_out, n, target, n))))
        return fail(LDM_ERR_BAD_ARG, "std_out must not overlap mean, m2 or target");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ensemble_finalize_kernel<>, dim3(nb), dim3(ENS_THREADS), 0, s, mean, m2, target, std_out, (EnsPartial*)scratch, (long)n,
                       (float)(count - ddof), ens_vec({mean, m2, target, std_out}));
    hipLaunchKernelGGL(ensemble_stats_kernel<>, dim3(1), dim3(ENS_THREADS), 0, s, (const EnsPartial*)scratch, nb, (double)n, target ? 1 : 0, stats);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- plan-only operator entries: the kernels that only the plan executor, ensure_derived and ensure_temb_table launch, through the
 * same helpers (launch_conv_thin, launch_split_f32, launch_x3_weights, launch_sinusoid, launch_gemv, launch_pack2, launch_pack_im2col,
 * guided_layout_launch, launch_phase_weights, launch_im2col_weights, launch_x3_phase_weights), for per-kernel tests against fp64.
 * They sit behind guided_layout_launch so that the guided template kernels keep their place in the code object. */
static int thin_args_ok(const void* x, const void* w, const void* out, int cin, int N, int D, int H, int W, int cout_real, int cout_pad) {
    if (!x || !w || !out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (N < 1 || D < 1 || H < 1 || W < 1 || (long)N * D * H * W >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad volume");
    if (cin < 32 || cin % 32) return fail(LDM_ERR_BAD_ARG, "cin must be a positive multiple of 32, got %d", cin);
    if (cout_real < 1 || cout_real > 4 || cout_pad < cout_real) return fail(LDM_ERR_BAD_ARG, "cout_real 1 .. 4 <= cout_pad, got %d / %d", cout_real, cout_pad);
    if (cin > 128) return fail(LDM_ERR_UNSUPPORTED, "conv3_thin_kernel is planned for at most 128 input channels, got %d", cin);
    return 0;
}
int ldm_op_conv3d_thin(const void* x, int cin, const void* w, const float* bias, float* out, int N, int D, int H, int W, int cout_real,
                       int cout_pad, void* stream) {
    LDM_TRY(thin_args_ok(x, w, out, cin, N, D, H, W, cout_real, cout_pad));
    ThinParams q{}; q.x = (const bf16_t*)x; q.w = (const bf16_t*)w; q.bias = bias; q.out = out;
    q.N = N; q.D = D; q.H = H; q.W = W; q.Cin = cin; q.CoutPad = cout_pad; q.CoutReal = cout_real;
    HIP_TRY(launch_conv_thin(q, (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
/* workspace of ldm_op_conv3d_thin_f32: the (hi | lo) split of x, then the [hi | lo | hi] weights */
static size_t thin_f32_split_bytes(int cin, int N, int D, int H, int W) { return rup_sz((size_t)N * D * H * W * 2 * cin * 2, 256); }
size_t ldm_op_conv3d_thin_f32_ws_bytes(int cin, int N, int D, int H, int W, int cout_pad) {
    if (cin < 1 || N < 1 || D < 1 || H < 1 || W < 1 || cout_pad < 1) { fail(LDM_ERR_BAD_ARG, "bad argument"); return 0; }
    return thin_f32_split_bytes(cin, N, D, H, W) + (size_t)27 * cout_pad * 3 * cin * 2;
}
int ldm_op_conv3d_thin_f32(const float* x, int cin, const float* w, const float* bias, float* out, int N, int D, int H, int W, int cout_real,
                           int cout_pad, void* ws, size_t ws_bytes, void* stream) {
    LDM_TRY(thin_args_ok(x, w, out, cin, N, D, H, W, cout_real, cout_pad));
    if (!ws || ws_bytes < ldm_op_conv3d_thin_f32_ws_bytes(cin, N, D, H, W, cout_pad)) return fail(LDM_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)ws % 16) return fail(LDM_ERR_BAD_ARG, "workspace not aligned to 16 bytes");
    hipStream_t s = (hipStream_t)stream;
    bf16_t* split = (bf16_t*)ws; bf16_t* w3 = (bf16_t*)((char*)ws + thin_f32_split_bytes(cin, N, D, H, W));
    launch_split_f32(x, split, N, cin, D, H, W, 0, s);
    launch_x3_weights(w, w3, 27L * cout_pad, cin, s);
    ThinParams q{}; q.x = split; q.w = w3; q.bias = bias; q.out = out;
    q.N = N; q.D = D; q.H = H; q.W = W; q.x3_c = cin; q.Cin = 3 * cin; q.CoutPad = cout_pad; q.CoutReal = cout_real;   // as OP_CONV_THIN fills it
    HIP_TRY(launch_conv_thin(q, s));
    HIP_TRY(hipGetLastError());
    return 0;
}
/* out[b][0 .. dim) = cos(t[b] f_j) | sin(t[b] f_j), f_j = exp(-ln(10000) j / (dim / 2)); an odd dim's last column is zero */
int ldm_op_timestep_embedding(const float* t, float* out, int B, int dim, void* stream) {
    if (!t || !out || B < 1 || dim < 2) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if ((long)B * dim > 4096L * 256) return fail(LDM_ERR_UNSUPPORTED, "temb_sinusoid_kernel writes one element per thread of at most 4096 blocks");
    launch_sinusoid(t, out, B, dim, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* y[b][o] = sum_i w[o][i] act(x[b][i]) + bias[o], act = SiLU when silu_in; w [O][I] bf16, or fp32 when fp32_weights; x rows x_stride
 * floats apart, y rows y_stride.  The kernels load whole 16-byte vectors: bf16 weights need I % 8 == 0; fp32 weights I % 4 == 0 and
 * x_stride % 4 == 0 (x is read as float4 too), and x 16-byte aligned. */
int ldm_op_gemv(const void* w, int fp32_weights, const float* bias, const float* x, float* y, int B, int I, int O, int x_stride, int y_stride,
                int silu_in, void* stream) {
    if (!w || !x || !y || B < 1 || B > 65535 || I < 1 || O < 1 || x_stride < I || y_stride < O) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if ((uintptr_t)w % 16) return fail(LDM_ERR_BAD_ARG, "weights not aligned to 16 bytes");
    if (fp32_weights ? (I % 4 || x_stride % 4 || (uintptr_t)x % 16) : I % 8)
        return fail(LDM_ERR_BAD_ARG, "16-byte row loads: I %% 8 == 0 (bf16 weights); I %% 4 == 0, x_stride %% 4 == 0, aligned x (fp32 weights)");
    launch_gemv(w, fp32_weights != 0, bias, x, y, B, I, O, x_stride, y_stride, silu_in ? 1 : 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* (x [N'][cx] | cond [N'][cc]) fp32 NCDHW -> out [N][DHW][Cs] (bf16, or fp32 when fp32_out), channels >= cx + cc zero.
 * guided_B = 0: N' = N.  guided_B = B > 0: the guided form, N must be 2 B and N' = B: samples 0 .. B-1 hold (x | fill), samples
 * B .. 2B-1 hold (x | cond). */
int ldm_op_pack2(const float* x, int cx, const float* cond, int cc, void* out, int N, int Cs, int64_t DHW, int fp32_out, int guided_B, float fill,
                 void* stream) {
    if (!cond) cc = 0;
    if (!x || !out || N < 1 || cx < 1 || cc < 0 || cx + cc > Cs || DHW < 1 || DHW >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (guided_B < 0 || (guided_B > 0 && (N != 2 * guided_B || cc < 1))) return fail(LDM_ERR_BAD_ARG, "the guided form needs N = 2 B and a condition tensor");
    hipStream_t s = (hipStream_t)stream;
    if (guided_B) {
        LayoutRec l{}; l.N = N; l.c_stored = Cs; l.DHW = (int)DHW;
        guided_layout_launch(fp32_out ? OP_PACK32 : OP_PACK, l, x, cx, cond, cc, fill, out, s);
    } else launch_pack2(x, cx, cond, cc, out, N, Cs, (int)DHW, fp32_out != 0, s);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The first conv's bf16 patch matrix out [N * D * H * W][Kp]: column tap * (cx + cc) + c holds input channel c of (x | cond) at the
 * voxel tap (kd, kh, kw) reads; out-of-volume taps and columns >= 27 (cx + cc) are zero.  guided_B as in ldm_op_pack2. */
int ldm_op_pack_im2col(const float* x, int cx, const float* cond, int cc, void* out, int N, int D, int H, int W, int Kp, int guided_B, float fill,
                       void* stream) {
    if (!cond) cc = 0;
    if (!x || !out || N < 1 || cx < 1 || cc < 0 || D < 1 || H < 1 || W < 1 || (long)N * D * H * W >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (Kp < 8 || Kp % 8 || Kp < 27 * (cx + cc)) return fail(LDM_ERR_BAD_ARG, "Kp %% 8 == 0 and Kp >= 27 (cx + cc), got %d", Kp);
    if (guided_B < 0 || (guided_B > 0 && (N != 2 * guided_B || cc < 1))) return fail(LDM_ERR_BAD_ARG, "the guided form needs N = 2 B and a condition tensor");
    hipStream_t s = (hipStream_t)stream;
    if (guided_B) {
        LayoutRec l{}; l.N = N; l.c_stored = Kp; l.D = D; l.H = H; l.W = W; l.DHW = D * H * W;
        guided_layout_launch(OP_IM2COL, l, x, cx, cond, cc, fill, out, s);
    } else launch_pack_im2col(x, cx, cond, cc, (bf16_t*)out, N, D, H, W, Kp, s);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* w3 bf16 [27][cout_pad][cin_s] -> wp bf16 [parity 8][tap 8][cout_pad][cin_s]: the taps of a (nearest x2 upsample -> 3^3 conv) that read
 * the same source voxel, summed in fp32 and rounded once (norm_elem.h phase_weights_kernel) */
int ldm_op_phase_weights(const void* w3, void* wp, int cout_pad, int cin_s, void* stream) {
    if (!w3 || !wp || cout_pad < 1 || cin_s < 8 || cin_s % 8) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_phase_weights((const bf16_t*)w3, (bf16_t*)wp, cout_pad, cin_s, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* w3 bf16 [27][cout_pad][cin_s] -> w2 bf16 [cout_pad][Kp], w2[co][tap * cin + c] = w3[tap][co][c], columns >= 27 cin zero */
int ldm_op_im2col_weights(const void* w3, void* w2, int cout_pad, int cin_s, int cin, int Kp, void* stream) {
    if (!w3 || !w2 || cout_pad < 1 || cin < 1 || cin > cin_s || Kp < 27 * cin || (long)cout_pad * Kp >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_im2col_weights((const bf16_t*)w3, (bf16_t*)w2, cout_pad, cin_s, cin, Kp, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* w fp32 [rows][cin] -> out bf16 [rows][hi(cin) | lo(cin) | hi(cin)], hi = bf16(w), lo = bf16(w - hi) */
int ldm_op_x3_weights(const float* w, void* out, int64_t rows, int cin, void* stream) {
    if (!w || !out || rows < 1 || cin < 4 || cin % 4) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_x3_weights(w, (bf16_t*)out, (long)rows, cin, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* w3 fp32 [27][cout_pad][cin] -> wp bf16 [parity 8][tap 8][cout_pad][hi | hi | lo] of the fp32 tap sums (f32_path.h x3_phase_weights_kernel) */
int ldm_op_x3_phase_weights(const float* w3, void* wp, int cout_pad, int cin, void* stream) {
    if (!w3 || !wp || cout_pad < 1 || cin < 4 || cin % 4) return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_x3_phase_weights(w3, (bf16_t*)wp, cout_pad, cin, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* x fp32 [N][D][H][W][C] -> out bf16 [N][D << up][H << up][W << up][hi(C) | lo(C)], nearest x2 upsampled when up = 1 */
int ldm_op_split_f32(const float* x, void* out, int N, int C, int D, int H, int W, int up, void* stream) {
    if (!x || !out || N < 1 || C < 4 || C % 4 || D < 1 || H < 1 || W < 1 || up < 0 || up > 1 || ((long)N * D * H * W << (3 * up)) >= (1L << 31))
        return fail(LDM_ERR_BAD_ARG, "bad argument");
    launch_split_f32(x, (bf16_t*)out, N, C, D, H, W, up, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- warm starts (warm_start.h): a chain that begins at row k0 of its sampler from a given latent --------------------------------
/* ldm_sampler_reset at row k0: step counter := k0, tbuf[0..B) := t of row k0.  0 <= k0 < n_steps; a PNDM sampler takes k0 = 0 only (its
 * warm-up and history are defined from the first row).  The Philox step index of a stochastic step stays the row index, so step k of a
 * warm chain draws the z that step k of the full chain draws. */
int ldm_sampler_seek(ldm_sampler* sp, int k0, float* tbuf, int B, void* stream) {
    if (!sp || !tbuf || B < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (k0 < 0 || k0 >= sp->n_steps) return fail(LDM_ERR_BAD_ARG, "start row %d outside 0 .. %d", k0, sp->n_steps - 1);
    if (sampler_multistep(sp) && k0 != 0)
        return fail(LDM_ERR_BAD_ARG, "a %s chain starts at its first row: k0 must be 0, got %d", sampler_multistep_name(sp), k0);
    hipLaunchKernelGGL(sampler_seek_kernel<0>, dim3(1), dim3(64), 0, (hipStream_t)stream, sp->st, (const float*)sp->coef,
                       sampler_row_len(sp), k0, tbuf, B);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int warm_start_check_shape(int B, int64_t per_sample) {
    if (B < 1 || B > 65535) return fail(LDM_ERR_BAD_ARG, "B must be in 1 .. 65535, got %d", B);
    if (per_sample < 1 || per_sample > ((int64_t)1 << 33)) return fail(LDM_ERR_BAD_ARG, "per_sample must be in 1 .. 2^33, got %lld", (long long)per_sample);
    return 0;
}
/* The noised start of a warm chain at row k0 of `sp` (DDPM, DDIM or rectified flow; PNDM is refused): x[b] = a z0[b or 0] + s e[b],
 * a = sqrt(abar_t), s = sqrt(1 - abar_t) of the row (flow: a = 1 - tau, s = tau), rounded as fma(a, z0, s * e).  z0_batch is 1 (one
 * latent for all B members, never copied) or B; e = noise [B][per_sample] or, with noise NULL, the Philox draw keyed by (seed, first_member
 * + b, element): warm_start.h.  x may alias z0 only when z0_batch == B. */
int ldm_sampler_start(const ldm_sampler* sp, int k0, const float* z0, int z0_batch, const float* noise, float* x, int B, int64_t per_sample,
                      uint64_t seed, uint32_t first_member, void* stream) {
    if (!sp || !z0 || !x) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(warm_start_check_shape(B, per_sample));
    if (sampler_multistep(sp)) return fail(LDM_ERR_BAD_ARG, "a %s chain has no warm start", sampler_multistep_name(sp));
    if (sp->repaint) return fail(LDM_ERR_BAD_ARG, "a repaint chain has no warm start");
    if (k0 < 0 || k0 >= sp->n_steps) return fail(LDM_ERR_BAD_ARG, "start row %d outside 0 .. %d", k0, sp->n_steps - 1);
    if (z0_batch != 1 && z0_batch != B) return fail(LDM_ERR_BAD_ARG, "z0_batch must be 1 or B = %d, got %d", B, z0_batch);
    if (x == z0 && z0_batch != B) return fail(LDM_ERR_BAD_ARG, "x may alias z0 only when z0_batch == B");
    if (noise == x) return fail(LDM_ERR_BAD_ARG, "x may not alias the noise");
    WarmStartParams p{};
    p.z0 = z0; p.noise = noise; p.x = x; p.row = sp->coef + (size_t)k0 * 8; p.per_sample = (long)per_sample; p.B = B; p.z0_batch = z0_batch;
    p.vec = lik_vec(per_sample, {z0, noise, x}); p.flow = sp->kind == SAMPLER_RFLOW ? 1 : 0;
    p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32); p.first_member = first_member;
    const dim3 grid(grid_for((long)((per_sample + 3) / 4) * B, 256, 1024));
    if (noise) hipLaunchKernelGGL(warm_start_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(warm_start_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* the N(0, 1) draws ldm_sampler_start(noise = NULL, seed) uses for global member `member` (tests: statistics, reproducibility) */
int ldm_sampler_start_noise(uint64_t seed, uint32_t member, float* out, int64_t per_sample, void* stream) {
    if (!out) return fail(LDM_ERR_BAD_ARG, "null argument");
    LDM_TRY(warm_start_check_shape(1, per_sample));
    hipLaunchKernelGGL(warm_start_noise_kernel<0>, dim3(grid_for((long)((per_sample + 3) / 4), 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       out, (long)per_sample, (unsigned)member, (unsigned)seed, (unsigned)(seed >> 32));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- inpainting (repaint.h): a chain that keeps the known part of a latent and regenerates the rest -------------------------------
// The device step of a repaint sampler (sampler_launch hands over; the entries have run repaint_check): the base family's update, the
// known-region merge and the jump back in one kernel, on the full latent or on the windows of `geom`.
static int repaint_launch(ldm_sampler* sp, const float* m, float* x, float* x0_out, int64_t n, float* tbuf, int B, hipStream_t s,
                          const WinGeom* geom, float* xw, int C) {
    LDM_TRY(repaint_check(sp, n, sp->rp_per_sample > 0 ? n / sp->rp_per_sample : 0));
    RepaintParams rp{};
    rp.s = step_params(sp); rp.s.m = m; rp.s.x = x; rp.s.x0_out = x0_out; rp.s.n = (long)n; rp.s.tbuf = tbuf; rp.s.B = B; rp.s.xw = xw; rp.s.C = C;
    rp.known = sp->known; rp.keep = sp->keep; rp.per_sample = (long)sp->rp_per_sample; rp.dhw = (long)sp->rp_dhw; rp.known_batch = sp->known_batch;
    const dim3 grid(grid_for((n + 3) / 4, 256, 1024));
    auto launch = [&](auto P, auto F) {
        if (!geom) hipLaunchKernelGGL((repaint_step_kernel<P(), F()>), grid, dim3(256), 0, s, rp);
        else hipLaunchKernelGGL((repaint_window_step_kernel<P(), F()>), grid, dim3(256), 0, s, *geom, rp);
    };
    if (sp->kind == SAMPLER_RFLOW) launch(std::integral_constant<int, PRED_EPSILON>{}, std::integral_constant<int, STEP_FLOW>{});
    else with_pred(sp->pred, [&](auto P) { launch(P, std::integral_constant<int, STEP_DDPM>{}); });
    return 0;
}
// what the merge and the jump ask of their four coefficients {ka, ks, ja, js} and the jump flag
static int repaint_check_coef(const float* c, float flags, int k) {
    for (int j = 0; j < 4; ++j) if (!std::isfinite(c[j])) return fail(LDM_ERR_BAD_ARG, "repaint row %d is not finite", k);
    if (flags != 0.f && flags != 1.f) return fail(LDM_ERR_BAD_ARG, "repaint row %d: the flags word must be 0 or 1 (jump), got %g", k, (double)flags);
    if (c[1] < 0.f || c[3] < 0.f) return fail(LDM_ERR_BAD_ARG, "repaint row %d: ks and js are standard deviations and may not be negative", k);
    if (c[3] != 0.f && flags == 0.f) return fail(LDM_ERR_BAD_ARG, "repaint row %d: js != 0 without the jump flag", k);
    return 0;
}
/* A repaint sampler: coef_host = [n_rows][LDM_REPAINT_ROW] fp32 rows, one per UNet call in sampling order (repaint.h): slots 0 .. 7 the
 * base scheduler's own row (kind 0 DDPM, 1 DDIM: as ldm_sampler_create takes them; 2 rectified flow: as ldm_sampler_create_rflow does),
 * then {ka, ks, ja, js, flags, 0, 0, 0}.  The timesteps (slot 5) need not fall.  At most LDM_REPAINT_MAX_ROWS rows
 * (LDM_ERR_UNSUPPORTED beyond): the time-embedding table of a denoising step has one row per UNet call. */
int ldm_sampler_create_repaint(const float* coef_host, int n_rows, int kind, int pred, int clip, uint64_t seed, ldm_sampler** out) {
    if (!coef_host || n_rows < 1 || kind < 0 || kind > 2 || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    static_assert(REPAINT_ROW == LDM_REPAINT_ROW, "row stride of the header");
    if (n_rows > LDM_REPAINT_MAX_ROWS) return fail(LDM_ERR_UNSUPPORTED, "a repaint chain of %d rows: at most %d are built", n_rows, LDM_REPAINT_MAX_ROWS);
    for (int k = 0; k < n_rows; ++k) {
        const float* r = coef_host + (size_t)k * REPAINT_ROW;
        for (int j = 0; j < REPAINT_ROW; ++j) if (!std::isfinite(r[j])) return fail(LDM_ERR_BAD_ARG, "repaint row %d is not finite", k);
        LDM_TRY(repaint_check_coef(r + 8, r[12], k));
    }
    std::unique_ptr<ldm_sampler> sp; LDM_TRY(sampler_alloc(coef_host, REPAINT_ROW, n_rows, &sp));
    sp->repaint = 1; sp->kind = kind == 2 ? (int)SAMPLER_RFLOW : kind;
    sp->pred = kind == 2 ? (int)PRED_EPSILON : pred; sp->clip = kind != 2 && clip ? 1 : 0;
    sp->seed_lo = (unsigned)seed; sp->seed_hi = (unsigned)(seed >> 32);
    *out = sp.release();
    return 0;
}
/* Hands a repaint sampler its caller-owned known latent [known_batch][per_sample] (known_batch 1: one latent for every sample, never
 * copied) and keep mask [dhw] (fp32, nonzero = keep; shared by the per_sample / dhw channels and by the samples); both must outlive
 * every step (and every recorded graph replay) that uses them.  Nothing is allocated or launched.  The sampler takes a new identity
 * in the graph cache, so no graph recorded on an earlier binding is replayed. */
int ldm_sampler_bind_known(ldm_sampler* sp, const float* known, int known_batch, const float* keep, int64_t per_sample, int64_t dhw) {
    if (!sp || !known || !keep) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (!sp->repaint) return fail(LDM_ERR_BAD_ARG, "only a repaint sampler takes a known latent");
    if (known_batch < 1 || known_batch > 65535) return fail(LDM_ERR_BAD_ARG, "known_batch must be in 1 .. 65535, got %d", known_batch);
    if (dhw < 1 || per_sample < dhw || per_sample % dhw || per_sample > ((int64_t)1 << 33))
        return fail(LDM_ERR_BAD_ARG, "per_sample (%lld) must be a multiple of dhw (%lld) in 1 .. 2^33", (long long)per_sample, (long long)dhw);
    sp->known = known; sp->keep = keep; sp->known_batch = known_batch; sp->rp_per_sample = per_sample; sp->rp_dhw = dhw;
    sp->uid = ++g_sampler_uid;
    return 0;
}
/* the N(0, 1) draws row `row` makes for a tensor of n elements on the known-region stream (which 0) or the jump stream (which 1) */
int ldm_sampler_repaint_noise(const ldm_sampler* sp, int which, int row, float* out, int64_t n, void* stream) {
    if (!sp || !out || n < 0 || row < 0 || which < 0 || which > 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (!sp->repaint) return fail(LDM_ERR_BAD_ARG, "not a repaint sampler");
    hipLaunchKernelGGL(repaint_noise_kernel<0>, dim3(grid_for((n + 3) / 4, 256, 1024)), dim3(256), 0, (hipStream_t)stream, out, (long)n,
                       (unsigned)row, which ? REPAINT_JUMP_STREAM_TAG : REPAINT_KNOWN_STREAM_TAG, sp->seed_lo, sp->seed_hi);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The host-driven merge and jump of one row on explicit draws, x / out [B][per_sample]: coef4_host = {ka, ks, ja, js} (HOST), jump 0 / 1;
 * the device step's per-element arithmetic (repaint_merge_jump), bit for bit.  z_known may be NULL when ks == 0, z_jump when jump == 0
 * or js == 0.  out may alias x. */
int ldm_repaint_merge(const float* x, const float* known, int known_batch, const float* keep, const float* z_known, const float* z_jump,
                      float* out, int B, int64_t per_sample, int64_t dhw, const float* coef4_host, int jump, void* stream) {
    if (!x || !known || !keep || !out || !coef4_host) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (B < 1 || B > 65535) return fail(LDM_ERR_BAD_ARG, "B must be in 1 .. 65535, got %d", B);
    if (dhw < 1 || per_sample < dhw || per_sample % dhw || per_sample > ((int64_t)1 << 33))
        return fail(LDM_ERR_BAD_ARG, "per_sample (%lld) must be a multiple of dhw (%lld) in 1 .. 2^33", (long long)per_sample, (long long)dhw);
    if (known_batch != 1 && known_batch != B) return fail(LDM_ERR_BAD_ARG, "known_batch must be 1 or B = %d, got %d", B, known_batch);
    if (jump != 0 && jump != 1) return fail(LDM_ERR_BAD_ARG, "jump must be 0 or 1, got %d", jump);
    LDM_TRY(repaint_check_coef(coef4_host, (float)jump, 0));
    if (coef4_host[1] != 0.f && !z_known) return fail(LDM_ERR_BAD_ARG, "ks != 0 needs z_known");
    if (jump && coef4_host[3] != 0.f && !z_jump) return fail(LDM_ERR_BAD_ARG, "a jump with js != 0 needs z_jump");
    RepaintMergeParams p{};
    p.x = x; p.known = known; p.keep = keep; p.zk = coef4_host[1] != 0.f ? z_known : nullptr; p.zj = jump && coef4_host[3] != 0.f ? z_jump : nullptr;
    p.out = out; p.n = (long)(B * per_sample); p.per_sample = (long)per_sample; p.dhw = (long)dhw; p.known_batch = known_batch;
    p.c = RepaintCoef{coef4_host[0], coef4_host[1], coef4_host[2], coef4_host[3], jump};
    hipLaunchKernelGGL(repaint_merge_kernel<0>, dim3(grid_for((p.n + 3) / 4, 256, 1024)), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- DPM-Solver++ (norm_elem.h STEP_DPM): the 2M multistep solver, ODE and SDE form, on the device sampler --------------------------
// The device step of a DPM-Solver++ sampler (sampler_launch hands over; it has run sampler_check_state): the one step loop with the DPM
// rule, on the full latent or on the windows of `geom`.
static int dpm_launch(ldm_sampler* sp, const float* m, float* x, float* x0_out, int64_t n, float* tbuf, int B, hipStream_t s,
                      const WinGeom* geom, float* xw, int C) {
    StepParams p = step_params(sp); p.m = m; p.x = x; p.x0_out = x0_out; p.n = (long)n; p.tbuf = tbuf; p.B = B; p.xw = xw; p.C = C;
    const dim3 grid(grid_for((n + 3) / 4, 256, 1024));
    with_pred(sp->pred, [&](auto P) {
        if (!geom) hipLaunchKernelGGL(dpm_sampler_step_kernel<P()>, grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL(dpm_window_step_kernel<P()>, grid, dim3(256), 0, s, *geom, p);
    });
    return 0;
}
// what the step asks of one row: finite, flags a whole number of known bits that agree with the coefficients they gate
static int dpm_check_row(const float* r, int k) {
    for (int j = 0; j < DPM_ROW; ++j) if (!std::isfinite(r[j])) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row %d is not finite", k);
    const DpmCoef c = dpm_coef(r);
    if (r[4] != (float)c.flags || c.flags < 0 || c.flags >= 8) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row %d: bad flags", k);
    if (c.cz < 0.f) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row %d: cz is a standard deviation and may not be negative", k);
    if (((c.flags & DPM_DRAWS) != 0) != (c.cz != 0.f)) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row %d: the DRAWS flag must be set exactly when cz != 0", k);
    if (!(c.flags & DPM_HAS_PREV) && c.c1 != 0.f) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row %d: c1 != 0 without the HAS_PREV flag", k);
    if ((c.flags & DPM_CLIP) && !(c.clip_min <= c.clip_max)) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row %d: clip_min above clip_max", k);
    return 0;
}
/* A DPM-Solver++ sampler (2M multistep; ODE and SDE form): coef_host = [n_steps][LDM_DPM_ROW] fp32 rows, one per UNet call in sampling
 * order (norm_elem.h: {cx, c0, sqrt(abar_s), sqrt(1 - abar_s), flags, t, c1, cz, 1/sqrt(abar_s), clip_min, clip_max, 0 ...}); pred 0
 * epsilon, 1 sample, 2 v_prediction.  The row program is replayed here once: a first row that reads the previous x0_hat, a non-finite
 * row, a negative cz and a DRAWS flag that disagrees with cz are refused, which is why the state buffer never needs zeroing and
 * ldm_sampler_reset (step counter := 0) rewinds the multistep state.  Noise: the sampler's Philox stream, counter = (element quad, row). */
int ldm_sampler_create_dpm(const float* coef_host, int n_steps, int pred, uint64_t seed, ldm_sampler** out) {
    if (!coef_host || n_steps < 1 || !out) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    static_assert(DPM_ROW == LDM_DPM_ROW && DPM_HAS_PREV == LDM_DPM_HAS_PREV && DPM_DRAWS == LDM_DPM_DRAWS && DPM_CLIP == LDM_DPM_CLIP,
                  "row layout of the header");
    for (int k = 0; k < n_steps; ++k) LDM_TRY(dpm_check_row(coef_host + (size_t)k * DPM_ROW, k));
    if ((int)coef_host[4] & DPM_HAS_PREV) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ row 0 reads the previous x0_hat before any row wrote one");
    std::unique_ptr<ldm_sampler> sp; LDM_TRY(sampler_alloc(coef_host, DPM_ROW, n_steps, &sp));
    sp->kind = SAMPLER_DPM; sp->pred = pred; sp->clip = 0; sp->seed_lo = (unsigned)seed; sp->seed_hi = (unsigned)(seed >> 32);
    *out = sp.release();
    return 0;
}
/* The host-driven DPM-Solver++ step (DPMSolverMultistepScheduler.step): one row of the table by value (row: LDM_DPM_ROW floats, as
 * ldm_sampler_create_dpm takes them), the previous x0_hat and the draw as explicit pointers; the device sampler's per-element arithmetic
 * (dpm_update), bit for bit.  x_out := the step of x with model output m; prev_x0_out and x0_out (each optional) := x0_hat.  prev_x0_in
 * may be NULL unless the row has HAS_PREV, z unless it has DRAWS; prev_x0_out may alias prev_x0_in.  x_out may not alias m or x. */
int ldm_dpm_step(const float* m, const float* x, const float* prev_x0_in, const float* z, float* prev_x0_out, float* x_out, float* x0_out,
                 int64_t n, int pred, const float* row, void* stream) {
    if (!m || !x || !x_out || !row || n < 0 || x_out == x || x_out == m) return fail(LDM_ERR_BAD_ARG, "bad argument");
    if (pred < PRED_EPSILON || pred > PRED_V) return fail(LDM_ERR_BAD_ARG, "unknown prediction type %d (0 epsilon, 1 sample, 2 v_prediction)", pred);
    LDM_TRY(dpm_check_row(row, 0));
    const DpmCoef c = dpm_coef(row);
    const bool has_prev = (c.flags & DPM_HAS_PREV) != 0, draws = (c.flags & DPM_DRAWS) != 0;
    if ((has_prev && !prev_x0_in) || (draws && !z)) return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ step: the row reads state or noise that was passed as NULL");
    const float* pi = has_prev ? prev_x0_in : nullptr; const float* zz = draws ? z : nullptr;
    if (x_out == pi || x_out == zz || (prev_x0_out && (prev_x0_out == x_out || prev_x0_out == m || prev_x0_out == x)) ||
        (x0_out && (x0_out == x_out || x0_out == m || x0_out == x || x0_out == pi)))
        return fail(LDM_ERR_BAD_ARG, "DPM-Solver++ step: an output aliases an input it may not");
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(grid_for((n + 3) / 4, 256, 1024));
    with_pred(pred, [&](auto P) { hipLaunchKernelGGL(dpm_step_kernel<P()>, g, dim3(256), 0, s, m, x, pi, zz, prev_x0_out, x_out, x0_out, (long)n, c); });
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- stage-2 objective (loss_weight.h): launched from here so that the kernel templates are emitted behind every older kernel
/* The weighted stage-2 loss, its gradient and the per-bin loss tracker in two launches (loss_weight.h); every refusal comes before any
 * launch. */
int ldm_op_weighted_mse_loss(const float* pred, const float* target, int B, int64_t per_sample, const int64_t* timesteps,
                             const float* w_table, int T, const float* sample_w, float* tracker, int K, float tracker_beta,
                             float* loss_out, float* per_sample_out, float* grad_out, void* stream) {
    if (!pred || !target || !loss_out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || per_sample < 1 || T < 1) return fail(LDM_ERR_BAD_ARG, "B %d, per_sample %lld and T %d must be positive", B, (long long)per_sample, T);
    if (B > LATENT_BATCH_MAX) return fail(LDM_ERR_UNSUPPORTED, "batch size %d above %d", B, LATENT_BATCH_MAX);
    if ((w_table || tracker) && !timesteps) return fail(LDM_ERR_BAD_ARG, "a weight table or a tracker needs the timesteps");
    if (K < 1 || K > LW_BINS_MAX || K > T) return fail(LDM_ERR_BAD_ARG, "K = %d bins outside 1 .. min(%d, T = %d)", K, (int)LW_BINS_MAX, T);
    if (tracker && !(tracker_beta >= 0.f && tracker_beta < 1.f)) return fail(LDM_ERR_BAD_ARG, "tracker_beta must lie in [0, 1)");
    float* parts = device_scratch(2, LW_PARTS_MAX * 4);
    if (!parts) return fail(LDM_ERR_HIP, "scratch allocation failed");
    LossWeightParams p{};
    p.pred = pred; p.target = target; p.grad = grad_out; p.parts = parts; p.timesteps = timesteps; p.w_table = w_table; p.sample_w = sample_w;
    p.per_sample = (long)per_sample; p.B = B; p.T = T; p.G = lw_vblocks((long)per_sample, B); p.rblocks = (p.G + 3) / 4;
    uintptr_t bits = (uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad_out;
    const bool vec = per_sample % 4 == 0 && (bits & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(lw_part_kernel<1>, dim3(B * p.rblocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(lw_part_kernel<0>, dim3(B * p.rblocks), dim3(256), 0, s, p);
    LossFoldParams f{};
    f.parts = parts; f.timesteps = timesteps; f.w_table = w_table; f.sample_w = sample_w; f.tracker = tracker; f.loss_out = loss_out;
    f.per_sample_out = per_sample_out; f.per_sample = (long)per_sample; f.B = B; f.T = T; f.K = K; f.G = p.G;
    f.w = lw_fold_slots(p.G); f.beta = tracker_beta;
    for (f.wlog = 0; (1 << f.wlog) < f.w; ++f.wlog) {}
    int fold_threads = (B * f.w + 63) / 64 * 64;                                      // one thread per slot, 128 .. 1024
    fold_threads = fold_threads < 128 ? 128 : (fold_threads > 1024 ? 1024 : fold_threads);
    hipLaunchKernelGGL(lw_fold_kernel<>, dim3(1), dim3(fold_threads), 0, s, f);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* The loss-aware draw of a batch's training timesteps and their importance weights in one launch (loss_weight.h).  idx is a HOST array
 * read before the call returns (only with draw NULL; NULL then means 0 .. B-1). */
int ldm_timestep_resample(const float* tracker, int K, int T, int warmup, float uniform_prob, const int* idx, int B, uint64_t seed,
                          uint32_t step, const float* draw, int64_t* t_out, float* iw_out, void* stream) {
    if (!tracker || !t_out || !iw_out) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (B < 1 || T < 1) return fail(LDM_ERR_BAD_ARG, "B %d and T %d must be positive", B, T);
    if (B > LATENT_BATCH_MAX) return fail(LDM_ERR_UNSUPPORTED, "batch size %d above %d", B, LATENT_BATCH_MAX);
    if (K < 1 || K > LW_BINS_MAX || K > T) return fail(LDM_ERR_BAD_ARG, "K = %d bins outside 1 .. min(%d, T = %d)", K, (int)LW_BINS_MAX, T);
    if (!(uniform_prob >= 0.f && uniform_prob <= 1.f)) return fail(LDM_ERR_BAD_ARG, "uniform_prob must lie in [0, 1]");
    ResampleParams p{};
    for (int b = 0; b < B; ++b) p.idx[b] = idx ? idx[b] : b;
    p.tracker = tracker; p.draw = draw; p.t_out = t_out; p.iw_out = iw_out; p.K = K; p.T = T; p.warmup = warmup; p.B = B;
    p.uniform_prob = uniform_prob; p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32); p.step = step;
    hipLaunchKernelGGL(lw_resample_kernel<>, dim3(1), dim3(LATENT_BATCH_MAX), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- gradients w.r.t. the UNet input and measurement-guided sampling: the kernels of conv_dgrad_thin.h and guidance.h are instantiated
// here, behind every kernel that was in the code object before them
#include "conv_dgrad_thin.h"
#include "guidance.h"
#include "guidance_image.h"
// conv3_dgrad_thin_kernel: q carries everything but the block counts; one 16-row tile for up to 16 real channels, two above
static void dgrad_thin_launch(const bf16_t* dy, const bf16_t* w, float* dx, float* dcond, int cx, int cc, int N, int D, int H, int W, int K, int x3_c,
                              hipStream_t s) {
    DgradThinParams q{}; q.dy = dy; q.w = w; q.dx = dx; q.dcond = dcond; q.cx = cx; q.cc = cc; q.N = N; q.D = D; q.H = H; q.W = W; q.K = K; q.x3_c = x3_c;
    q.td = (q.D + THIN_TD - 1) / THIN_TD; q.th = (q.H + THIN_TH - 1) / THIN_TH; q.tw = (q.W + THIN_TW - 1) / THIN_TW;
    const dim3 grid((unsigned)((long)q.N * q.td * q.th * q.tw));
    if (q.cx + q.cc <= 16) hipLaunchKernelGGL(conv3_dgrad_thin_kernel<1>, grid, dim3(256), THIN_LDS_X, s, q);
    else hipLaunchKernelGGL(conv3_dgrad_thin_kernel<2>, grid, dim3(256), THIN_LDS_X, s, q);
}
// its weights [27 mirrored taps][32][K] from w(co, ci, tap) at co s_co + ci s_ci + tap s_tap (fp32 or bf16 source); x3: K = 3 C, [hi | lo | hi]
static void launch_dgrad_thin_pack(const void* w, bool src_f32, bf16_t* wp, int cout, int cin_real, int K, bool x3, long s_co, long s_ci, long s_tap,
                                   hipStream_t s) {
    const dim3 grid(grid_for(27L * 32 * K, 256, 1024));
    if (src_f32) hipLaunchKernelGGL(dgrad_thin_pack_kernel<float>, grid, dim3(256), 0, s, (const float*)w, wp, cout, cin_real, K, x3 ? 1 : 0, s_co, s_ci, s_tap);
    else hipLaunchKernelGGL(dgrad_thin_pack_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)w, wp, cout, cin_real, K, x3 ? 1 : 0, s_co, s_ci, s_tap);
}

extern "C" {

/* Thin data gradient of a 3^3 stride-1 pad-1 conv with 1 .. 32 real input channels (conv_dgrad_thin.h), from the conv's own fp32
 * [Cout][Cin][3][3][3] weight: packs it (rounded to bf16, or split hi | lo in fp32 mode) and launches, as the backward plans do.
 * The packed weights (and the split of dy in fp32 mode) live in a buffer allocated and freed here: a test entry, it synchronises. */
int ldm_op_conv3d_dgrad_thin(const void* dy, int cdy, const float* w, int cout, int cin_real, int cx, int cc, float* dx, float* dcond,
                             int N, int D, int H, int W, int fp32_mode, void* stream) {
    if (!dy || !w || (!dx && !dcond)) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (cdy < 32 || cdy % 32 || cout < 1 || cout > cdy) return fail(LDM_ERR_BAD_ARG, "cdy must be a positive multiple of 32 and >= cout");
    if (cin_real < 1 || cin_real > 32 || cx < 0 || cc < 0 || cx + cc != cin_real) return fail(LDM_ERR_BAD_ARG, "cx + cc = cin_real in 1 .. 32, got %d + %d / %d", cx, cc, cin_real);
    if (N < 1 || D < 1 || H < 1 || W < 1 || (long)N * D * H * W >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad volume");
    hipStream_t s = (hipStream_t)stream;
    const int K = fp32_mode ? 3 * cdy : cdy;
    const size_t wp_bytes = rup_sz((size_t)27 * 32 * K * 2, 256), split_bytes = fp32_mode ? (size_t)N * D * H * W * 2 * cdy * 2 : 0;
    char* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, wp_bytes + split_bytes));
    launch_dgrad_thin_pack(w, true, (bf16_t*)buf, cout, cin_real, K, fp32_mode != 0, 27L * cin_real, 27, 1, s);
    if (fp32_mode) launch_split_f32((const float*)dy, (bf16_t*)(buf + wp_bytes), N, cdy, D, H, W, 0, s);
    dgrad_thin_launch(fp32_mode ? (const bf16_t*)(buf + wp_bytes) : (const bf16_t*)dy, (const bf16_t*)buf, dx, dcond, cx, cc, N, D, H, W, K,
                      fp32_mode ? cdy : 0, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(buf);
    HIP_TRY(e);
    return 0;
}
/* The two halves of the entry above on caller-owned memory, nothing allocated or synchronised (timing, tools/bench_guided_step.py):
 * the re-pack into wp, 27 * 32 * K bf16 with K = cdy (fp32_mode: 3 cdy), and the kernel alone on packed weights.  fp32_mode: dy is the
 * (hi | lo) bf16 split [N*D*H*W][2 cdy] of the fp32 gradient. */
int ldm_op_conv3d_dgrad_thin_pack(const float* w, int cdy, int cout, int cin_real, int fp32_mode, void* wp, void* stream) {
    if (!w || !wp) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (cdy < 32 || cdy % 32 || cout < 1 || cout > cdy || cin_real < 1 || cin_real > 32) return fail(LDM_ERR_BAD_ARG, "bad channel counts");
    launch_dgrad_thin_pack(w, true, (bf16_t*)wp, cout, cin_real, fp32_mode ? 3 * cdy : cdy, fp32_mode != 0, 27L * cin_real, 27, 1, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
int ldm_op_conv3d_dgrad_thin_packed(const void* dy, int cdy, const void* wp, int cx, int cc, float* dx, float* dcond,
                                    int N, int D, int H, int W, int fp32_mode, void* stream) {
    if (!dy || !wp || (!dx && !dcond)) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (cdy < 32 || cdy % 32 || cx < 0 || cc < 0 || cx + cc < 1 || cx + cc > 32) return fail(LDM_ERR_BAD_ARG, "bad channel counts");
    if (N < 1 || D < 1 || H < 1 || W < 1 || (long)N * D * H * W >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad volume");
    dgrad_thin_launch((const bf16_t*)dy, (const bf16_t*)wp, dx, dcond, cx, cc, N, D, H, W, fp32_mode ? 3 * cdy : cdy, fp32_mode ? cdy : 0,
                      (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- measurement-guided sampling (guidance.h) ---- */
static int guidance_shape_ok(int pred, int pool, int target_batch, int weight_batch, bool has_weight, int B, int C, int D, int H, int W) {
    if (pred != PRED_EPSILON && pred != PRED_SAMPLE && pred != PRED_V) return fail(LDM_ERR_BAD_ARG, "prediction type must be 0, 1 or 2, got %d", pred);
    if (B < 1 || B > 65535 || C < 1 || D < 1 || H < 1 || W < 1 || (long)C * D * H * W >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad shape");
    if (pool < 1 || D % pool || H % pool || W % pool) return fail(LDM_ERR_BAD_ARG, "pool %d must divide the latent dims %d x %d x %d", pool, D, H, W);
    if (target_batch != 1 && target_batch != B) return fail(LDM_ERR_BAD_ARG, "target_batch must be 1 or %d, got %d", B, target_batch);
    if (has_weight && weight_batch != 1 && weight_batch != B) return fail(LDM_ERR_BAD_ARG, "weight_batch must be 1 or %d, got %d", B, weight_batch);
    return 0;
}
static void guidance_residual_launch(const GuideResParams& p, hipStream_t s) {
    hipLaunchKernelGGL(guidance_residual_kernel, dim3(p.B), dim3(256), 0, s, p);
}
static void guidance_update_launch(float* x, const float* gx, const float* dx, const float* norm2, float scale, int normalize, int64_t per_sample, int B,
                                   hipStream_t s) {
    hipLaunchKernelGGL(guidance_update_kernel, dim3(grid_for(per_sample * B, 256, 1024)), dim3(256), 0, s, x, gx, dx, norm2, scale, normalize,
                       (long)per_sample, B);
}
/* The residual kernel on its own, sqrt(abar_t) and sqrt(1 - abar_t) by value: grad_out := c_m g, gx := c_x g (both [B][C][D][H][W]),
 * norm2[b] := |r_b|^2 (deterministic).  target [target_batch][C][D/p][H/p][W/p], weight the same shape per sample or NULL. */
int ldm_op_guidance_residual(const float* x, const float* m, const float* target, int target_batch, const float* weight, int weight_batch,
                             float sqrt_abar, float sqrt_one_minus_abar, int pred, int pool, float* grad_out, float* gx, float* norm2,
                             int B, int C, int D, int H, int W, void* stream) {
    if (!x || !m || !target || !grad_out || !gx || !norm2) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    if (!(sqrt_abar > 0.f)) return fail(LDM_ERR_BAD_ARG, "sqrt(abar) must be positive");
    LDM_TRY(guidance_shape_ok(pred, pool, target_batch, weight_batch, weight != nullptr, B, C, D, H, W));
    GuideResParams p{}; p.x = x; p.m = m; p.target = target; p.target_batch = target_batch; p.weight = weight; p.weight_batch = weight_batch;
    p.grad_out = grad_out; p.gx = gx; p.norm2 = norm2; p.a = sqrt_abar; p.s = sqrt_one_minus_abar;
    p.pred = pred; p.pool = pool; p.B = B; p.C = C; p.D = D; p.H = H; p.W = W;
    guidance_residual_launch(p, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* x -= zeta_b (gx + dx) in place, zeta_b = scale / max(sqrt(norm2[b]), 1e-12) (normalize) or scale; norm2 is read on the device. */
int ldm_op_guidance_update(float* x, const float* gx, const float* dx, const float* norm2, float scale, int normalize, int B, int64_t per_sample,
                           void* stream) {
    if (!x || !gx || !dx || !norm2 || B < 1 || per_sample < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    guidance_update_launch(x, gx, dx, norm2, scale, normalize, per_sample, B, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* One measurement-guided denoising step on a DDPM / DDIM sampler, five launches groups in this order: the training forward (m = UNet(x_t)
 * into eps_scratch, tape in `workspace`), the residual kernel (row = the sampler's device step counter), the data-only input backward
 * (g->dx := J^T(c_m g)), ldm_sampler_step (x in place, counter and tbuf advance), the update kernel.  The host reads nothing; g->norm_table
 * (optional, [n_steps][B]) receives |r_b| of the step.  The arguments, the sampler's kind, the channel split the thin data gradient will
 * see, both plans and the workspace are checked in front of the forward; what the later launches check again cannot fail after that
 * (a DDPM / DDIM sampler without inpainting binds no state and takes any element count).  workspace:
 * ldm_unet_train_input_workspace_bytes.  Not graph-replayed. */
int ldm_unet_denoise_step_measured(ldm_model* m, ldm_sampler* sp, const ldm_measurement* g, float* x, int x_channels, const float* cond,
                                   int cond_channels, float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!sp || !g || !x || !tbuf || !eps_scratch) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (sp->kind > SAMPLER_DDIM || sp->repaint) return fail(LDM_ERR_UNSUPPORTED, "measurement guidance runs on a DDPM or DDIM sampler without inpainting");
    if (sp->n_steps > 1 && sp->ts.front() < sp->ts.back())
        return fail(LDM_ERR_UNSUPPORTED, "measurement guidance runs on a denoising sampler: this one's timesteps ascend (DDIM inversion)");
    if (B < 1 || D < 1 || H < 1 || W < 1) return fail(LDM_ERR_BAD_ARG, "bad shape");
    if (x_channels != m->ucfg.out_channels) return fail(LDM_ERR_BAD_ARG, "x must have the UNet's out_channels (%d)", m->ucfg.out_channels);
    if (!cond) cond_channels = 0;
    if (x_channels + cond_channels != m->ucfg.in_channels)
        return fail(LDM_ERR_BAD_ARG, "x_channels + cond_channels = %d, model expects %d", x_channels + cond_channels, m->ucfg.in_channels);
    if (!g->target || !g->grad_out || !g->gx || !g->dx || !g->norm2) return fail(LDM_ERR_BAD_ARG, "measurement: null tensor");
    LDM_TRY(guidance_shape_ok(sp->pred, g->pool, g->target_batch, g->weight_batch, g->weight != nullptr, B, x_channels, D, H, W));
    {   // both plans and the workspace, before the forward runs
        std::shared_ptr<Plan> p;
        LDM_TRY(ready_plan(m, "train", B, D, H, W, workspace, workspace_bytes, &p));
        LDM_TRY(ready_plan(m, "train_x", B, D, H, W, workspace, workspace_bytes, &p));
    }
    hipStream_t s = (hipStream_t)stream;
    LDM_TRY(ldm_unet_train_forward(m, x, x_channels, cond, cond_channels, tbuf, eps_scratch, B, D, H, W, workspace, workspace_bytes, stream));
    GuideResParams p{}; p.x = x; p.m = eps_scratch; p.target = g->target; p.target_batch = g->target_batch; p.weight = g->weight;
    p.weight_batch = g->weight_batch; p.grad_out = g->grad_out; p.gx = g->gx; p.norm2 = g->norm2; p.norm_tab = g->norm_table;
    p.coef = sp->coef; p.st = sp->st; p.n_steps = sp->n_steps; p.a = 1.f;
    p.pred = sp->pred; p.pool = g->pool; p.B = B; p.C = x_channels; p.D = D; p.H = H; p.W = W;
    guidance_residual_launch(p, s);
    LDM_TRY(ldm_unet_train_backward_input(m, g->grad_out, nullptr, g->dx, nullptr, B, D, H, W, workspace, workspace_bytes, stream));
    const int64_t per = (int64_t)x_channels * D * H * W;
    LDM_TRY(sampler_launch(sp, eps_scratch, x, nullptr, per * B, tbuf, B, s));
    guidance_update_launch(x, g->gx, g->dx, g->norm2, g->scale, g->normalize, per, B, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- image-space measurement guidance (guidance_image.h) ---- */
static int image_residual_shape_ok(int pool, int target_batch, int weight_batch, bool has_weight, int B, int C, int D, int H, int W) {
    if (B < 1 || B > 65535 || C < 1 || D < 1 || H < 1 || W < 1 || (long)C * D * H * W >= (1L << 31)) return fail(LDM_ERR_BAD_ARG, "bad shape");
    if (pool < 1 || pool > 1024 || D % pool || H % pool || W % pool)
        return fail(LDM_ERR_BAD_ARG, "pool %d must be in [1, 1024] and divide the image dims %d x %d x %d", pool, D, H, W);
    if (target_batch != 1 && target_batch != B) return fail(LDM_ERR_BAD_ARG, "target_batch must be 1 or %d, got %d", B, target_batch);
    if (has_weight && weight_batch != 1 && weight_batch != B) return fail(LDM_ERR_BAD_ARG, "weight_batch must be 1 or %d, got %d", B, weight_batch);
    return 0;
}
static int guide_coef_ok(int pred, float sqrt_abar) {
    if (pred != PRED_EPSILON && pred != PRED_SAMPLE && pred != PRED_V) return fail(LDM_ERR_BAD_ARG, "prediction type must be 0, 1 or 2, got %d", pred);
    if (!(sqrt_abar > 0.f)) return fail(LDM_ERR_BAD_ARG, "sqrt(abar) must be positive");
    return 0;
}
static void guidance_x0_launch(const float* x, const float* m, float* z0, const GuideCoefSrc& g, float inv_sf, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(guidance_x0_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, x, m, z0, g, inv_sf, (long)n);
}
static void guidance_chain_launch(const float* dz, float* grad_out, float* gx, const GuideCoefSrc& g, float inv_sf, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(guidance_chain_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, dz, grad_out, gx, g, inv_sf, (long)n);
}
// the residual kernel and its fold; st / n_steps: the sampler's device step counter and row count behind norm_tab (or null)
static void image_residual_launch(ImageResParams p, int B, float* norm2, float* norm_tab, const SamplerState* st, int n_steps, hipStream_t s) {
    p.geom = image_residual_geom(p.C, p.D, p.H, p.W, p.pool);
    hipLaunchKernelGGL(image_residual_kernel, dim3((unsigned)p.geom.chunks, B), dim3(256), 0, s, p);
    hipLaunchKernelGGL(image_residual_fold_kernel, dim3(B), dim3(64), 0, s, (const double*)p.partials, p.geom.chunks, norm2, norm_tab, st, n_steps, B);
}
/* Bytes of the `partials` scratch of ldm_op_image_residual and of ldm_image_measurement: one double per (sample, chunk), the chunk count
 * a function of the shape alone.  0 (with an error message) for a shape the kernel refuses. */
size_t ldm_image_residual_scratch_bytes(int B, int C, int D, int H, int W, int pool) {
    if (image_residual_shape_ok(pool, 1, 1, false, B, C, D, H, W)) return 0;
    return (size_t)B * image_residual_geom(C, D, H, W, pool).chunks * sizeof(double);
}
/* z0 := x0_hat(x, m) * inv_scale_factor over n elements, sqrt(abar_t) and sqrt(1 - abar_t) by value. */
int ldm_op_guidance_x0(const float* x, const float* m, float sqrt_abar, float sqrt_one_minus_abar, int pred, float inv_scale_factor, float* z0,
                       int64_t n, void* stream) {
    if (!x || !m || !z0 || n < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    LDM_TRY(guide_coef_ok(pred, sqrt_abar));
    GuideCoefSrc g{}; g.a = sqrt_abar; g.s = sqrt_one_minus_abar; g.pred = pred;
    guidance_x0_launch(x, m, z0, g, inv_scale_factor, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* g_img := pool^-3 upsample_nearest(w .* r), norm2[b] := |r_b|^2 for r = w .* (P y_hat - target) on an image [B][C][D][H][W]; g_img may
 * alias y_hat.  partials: ldm_image_residual_scratch_bytes, 8-byte aligned.  Deterministic, and slot b does not depend on B. */
int ldm_op_image_residual(const float* y_hat, const float* target, int target_batch, const float* weight, int weight_batch, int pool,
                          float* g_img, float* norm2, void* partials, size_t partials_bytes, int B, int C, int D, int H, int W, void* stream) {
    if (!y_hat || !target || !g_img || !norm2 || !partials) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    LDM_TRY(image_residual_shape_ok(pool, target_batch, weight_batch, weight != nullptr, B, C, D, H, W));
    if (partials_bytes < ldm_image_residual_scratch_bytes(B, C, D, H, W, pool) || ((uintptr_t)partials & 7))
        return fail(LDM_ERR_WORKSPACE, "partials: need %zu bytes, 8-byte aligned", ldm_image_residual_scratch_bytes(B, C, D, H, W, pool));
    ImageResParams p{}; p.y_hat = y_hat; p.target = target; p.target_batch = target_batch; p.weight = weight; p.weight_batch = weight_batch;
    p.g_img = g_img; p.partials = (double*)partials; p.pool = pool; p.C = C; p.D = D; p.H = H; p.W = W;
    image_residual_launch(p, B, norm2, nullptr, nullptr, 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* grad_out := c_m dz * inv_scale_factor, gx := c_x dz * inv_scale_factor over n elements, coefficients by value. */
int ldm_op_guidance_chain(const float* dz, float sqrt_abar, float sqrt_one_minus_abar, int pred, float inv_scale_factor, float* grad_out, float* gx,
                          int64_t n, void* stream) {
    if (!dz || !grad_out || !gx || n < 1) return fail(LDM_ERR_BAD_ARG, "bad argument");
    LDM_TRY(guide_coef_ok(pred, sqrt_abar));
    GuideCoefSrc g{}; g.a = sqrt_abar; g.s = sqrt_one_minus_abar; g.pred = pred;
    guidance_chain_launch(dz, grad_out, gx, g, inv_scale_factor, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* One image-space measurement-guided step: UNet training forward -> x0 kernel (z0 := x0_hat / sf) -> decoder grad-forward (recon :=
 * Dec(z0)) -> image residual and fold (recon := g_img in place) -> decoder data-only backward (dz) -> chain kernel -> UNet data-only input
 * backward (dx) -> ldm_sampler_step -> update kernel.  The refusals of ldm_unet_denoise_step_measured, and: `vae` must be an AutoencoderKL
 * whose latent_channels equal x_channels, the target is [target_batch][out_channels][Di/pool][Hi/pool][Wi/pool] on the image dims
 * (Di, Hi, Wi) = (D, H, W) * 2^(levels - 1).  Every argument, all plans of both models and both workspaces are checked before the first
 * launch; the host reads nothing.  workspace: ldm_unet_train_input_workspace_bytes; g->vae_workspace:
 * ldm_vae_decode_grad_workspace_bytes.  Not graph-replayed. */
int ldm_unet_denoise_step_measured_image(ldm_model* m, ldm_model* vae, ldm_sampler* sp, const ldm_image_measurement* g, float* x, int x_channels,
                                         const float* cond, int cond_channels, float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || m->type != 0) return fail(LDM_ERR_BAD_ARG, "not a UNet handle");
    if (!vae || vae->type != 1) return fail(LDM_ERR_BAD_ARG, "vae: not an AutoencoderKL handle");
    if (!sp || !g || !x || !tbuf || !eps_scratch) return fail(LDM_ERR_BAD_ARG, "null argument");
    if (sp->kind > SAMPLER_DDIM || sp->repaint) return fail(LDM_ERR_UNSUPPORTED, "measurement guidance runs on a DDPM or DDIM sampler without inpainting");
    if (sp->n_steps > 1 && sp->ts.front() < sp->ts.back())
        return fail(LDM_ERR_UNSUPPORTED, "measurement guidance runs on a denoising sampler: this one's timesteps ascend (DDIM inversion)");
    if (B < 1 || D < 1 || H < 1 || W < 1) return fail(LDM_ERR_BAD_ARG, "bad shape");
    if (x_channels != m->ucfg.out_channels) return fail(LDM_ERR_BAD_ARG, "x must have the UNet's out_channels (%d)", m->ucfg.out_channels);
    if (x_channels != vae->vcfg.latent_channels)
        return fail(LDM_ERR_BAD_ARG, "the AutoencoderKL's latent_channels (%d) must equal x_channels (%d)", vae->vcfg.latent_channels, x_channels);
    if (!cond) cond_channels = 0;
    if (x_channels + cond_channels != m->ucfg.in_channels)
        return fail(LDM_ERR_BAD_ARG, "x_channels + cond_channels = %d, model expects %d", x_channels + cond_channels, m->ucfg.in_channels);
    if (!g->target || !g->z0 || !g->recon || !g->dz || !g->grad_out || !g->gx || !g->dx || !g->norm2 || !g->partials)
        return fail(LDM_ERR_BAD_ARG, "measurement: null tensor");
    if (!(g->inv_scale_factor > 0.f)) return fail(LDM_ERR_BAD_ARG, "measurement: inv_scale_factor must be positive");
    if (sp->pred != PRED_EPSILON && sp->pred != PRED_SAMPLE && sp->pred != PRED_V) return fail(LDM_ERR_BAD_ARG, "prediction type must be 0, 1 or 2, got %d", sp->pred);
    const int f = 1 << (vae->vcfg.num_levels - 1), Ci = vae->vcfg.out_channels;
    if ((long)D * f > 2040 || (long)H * f > 2040 || (long)W * f > 2040) return fail(LDM_ERR_BAD_ARG, "bad shape");
    const int Di = D * f, Hi = H * f, Wi = W * f;
    LDM_TRY(image_residual_shape_ok(g->pool, g->target_batch, g->weight_batch, g->weight != nullptr, B, Ci, Di, Hi, Wi));
    if (((uintptr_t)g->partials) & 7) return fail(LDM_ERR_BAD_ARG, "measurement: partials must be 8-byte aligned");
    {   // every plan of both models and both workspaces, before the forward runs
        std::shared_ptr<Plan> p;
        LDM_TRY(ready_plan(m, "train", B, D, H, W, workspace, workspace_bytes, &p));
        LDM_TRY(ready_plan(m, "train_x", B, D, H, W, workspace, workspace_bytes, &p));
        LDM_TRY(ready_plan(vae, "dec_x", B, D, H, W, g->vae_workspace, g->vae_workspace_bytes, &p));
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t per = (int64_t)x_channels * D * H * W;
    GuideCoefSrc cs{}; cs.coef = sp->coef; cs.st = sp->st; cs.n_steps = sp->n_steps; cs.a = 1.f; cs.pred = sp->pred;
    LDM_TRY(ldm_unet_train_forward(m, x, x_channels, cond, cond_channels, tbuf, eps_scratch, B, D, H, W, workspace, workspace_bytes, stream));
    guidance_x0_launch(x, eps_scratch, g->z0, cs, g->inv_scale_factor, per * B, s);
    LDM_TRY(ldm_vae_decode_grad_forward(vae, g->z0, g->recon, B, D, H, W, g->vae_workspace, g->vae_workspace_bytes, stream));
    ImageResParams p{}; p.y_hat = g->recon; p.target = g->target; p.target_batch = g->target_batch; p.weight = g->weight; p.weight_batch = g->weight_batch;
    p.g_img = g->recon; p.partials = (double*)g->partials; p.pool = g->pool; p.C = Ci; p.D = Di; p.H = Hi; p.W = Wi;
    image_residual_launch(p, B, g->norm2, g->norm_table, sp->st, sp->n_steps, s);
    LDM_TRY(ldm_vae_decode_grad_backward(vae, g->recon, g->dz, B, D, H, W, g->vae_workspace, g->vae_workspace_bytes, stream));
    guidance_chain_launch(g->dz, g->grad_out, g->gx, cs, g->inv_scale_factor, per * B, s);
    LDM_TRY(ldm_unet_train_backward_input(m, g->grad_out, nullptr, g->dx, nullptr, B, D, H, W, workspace, workspace_bytes, stream));
    LDM_TRY(sampler_launch(sp, eps_scratch, x, nullptr, per * B, tbuf, B, s));
    guidance_update_launch(x, g->gx, g->dx, g->norm2, g->scale, g->normalize, per, B, s);
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // extern "C"

// ---- gradient accumulation over micro-batches (grad_accum.h): instantiated here, behind every kernel that was
// in the code object before it
#include "grad_accum.h"
static int grad_accum_launch(float* acc, const float* g, int64_t n, float scale, int assign, hipStream_t s) {
    if (n <= 0) return 0;
    // acc and g share their misalignment inside the flat buffers; a pair that does not (or is not float-aligned) runs scalar throughout
    const uintptr_t pa = (uintptr_t)acc, pg = (uintptr_t)g;
    long head = (pa ^ pg) & 15 || (pa & 3) ? (long)n : (long)(((16 - (pa & 15)) & 15) / 4);
    if (head > n) head = (long)n;
    const long nvec = ((long)n - head) / 4, tail = (long)n - head - 4 * nvec;
    const dim3 grid(grid_for(nvec > head + tail ? nvec : head + tail, 256, 2048));
    // the project's launch timeline (ldm_profile_start(LDM_PROFILE_GRAD_ACCUM, ...)): events around every accumulate launch
    const bool hit = g_prof.on && g_prof.wgm == LDM_PROFILE_GRAD_ACCUM && g_prof.used + 2 <= g_prof.ev.size();
    if (hit) HIP_TRY(hipEventRecord(g_prof.ev[g_prof.used], s));
    if (assign) hipLaunchKernelGGL(grad_accum_kernel<true>, grid, dim3(256), 0, s, acc, g, head, nvec, tail, scale);
    else hipLaunchKernelGGL(grad_accum_kernel<false>, grid, dim3(256), 0, s, acc, g, head, nvec, tail, scale);
    if (hit) {            // "flops" of the timeline = the bytes the pass moves: 8 per element (assign), 12 (add)
        HIP_TRY(hipEventRecord(g_prof.ev[g_prof.used + 1], s)); g_prof.used += 2; g_prof.flops.push_back((double)n * (assign ? 8.0 : 12.0));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

/* acc[i] = g[i] * scale (assign != 0; acc is not read) or acc[i] += g[i] * scale over n fp32 elements, one streaming launch
 * (grad_accum.h).  n == 0: nothing is launched. */
int ldm_op_grad_accumulate(float* acc, const float* g, int64_t n, float scale, int assign, void* stream) {
    if (n < 0) return fail(LDM_ERR_BAD_ARG, "n < 0");
    if (n == 0) return 0;
    if (!acc || !g) return fail(LDM_ERR_BAD_ARG, "null tensor argument");
    return grad_accum_launch(acc, g, n, scale, assign, (hipStream_t)stream);
}

/* Arm (acc_flat != NULL) or disarm (NULL) gradient accumulation for the training backwards of a UNet or AutoencoderKL handle: this
 * backward is micro-batch `micro_index` of a window of `micro_count`.  See include/ldm3d.h.  Bad arguments leave the previous setting. */
int ldm_model_set_grad_accum(ldm_model* m, float* acc_flat, int micro_index, int micro_count) {
    if (!m) return fail(LDM_ERR_BAD_ARG, "null model");
    if (!acc_flat) { m->gaccum = GradAccumState(); return 0; }
    if (micro_count < 1 || micro_index < 0 || micro_index >= micro_count)
        return fail(LDM_ERR_BAD_ARG, "gradient accumulation: need micro_count >= 1 and 0 <= micro_index < micro_count, got %d of %d", micro_index, micro_count);
    m->gaccum.acc = acc_flat; m->gaccum.micro = micro_index; m->gaccum.count = micro_count;
    return 0;
}
}  // extern "C"
