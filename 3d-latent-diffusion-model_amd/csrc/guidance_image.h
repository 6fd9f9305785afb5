// Image-space measurement guidance: the element-wise kernels around the decoder's and the UNet's input VJPs for
// the weighted pooled quadratic on the DECODED prediction.  sf = the inferer's scale_factor, Dec = the AutoencoderKL decoder:
//   x0_hat = (x - s m) / a (epsilon) | m (sample) | a x - s m (v_prediction), UNCLIPPED;  z0 = x0_hat / sf;  y_hat = Dec(z0)
//   r = w .* (P y_hat - y), P = mean over non-overlapping pool^3 cubes of the IMAGE per image channel;  L_b = 1/2 |r_b|^2
//   g_img = dL/dy_hat = pool^-3 upsample_nearest(w .* r);  dz = Dec'^T g_img;  grad_x L = c_x (dz / sf) + J^T(c_m (dz / sf))
// guidance_x0_kernel writes z0; image_residual_kernel writes g_img and one double partial of |r_b|^2 per (sample, chunk);
// image_residual_fold_kernel adds a sample's partials in index order; guidance_chain_kernel writes c_m dz / sf (the grad_out of the UNet's
// data-only backward) and c_x dz / sf.  guidance_update_kernel (guidance.h) finishes the step.
//
// image_residual_kernel works on tiles: the pool x pool image rows behind `cw` neighbouring cubes of one cube row (c, qd, qh).  Every global
// read of y_hat and write of g_img walks a row segment of cw * pool contiguous floats, lane after lane (pool == 1: a chunk is a contiguous
// run of voxels); the rows are staged through LDS, summed per row by (row, cube) pairs and per cube in row order.  The geometry (cw, tiles
// per chunk, chunk count) is a function of the shape alone (image_residual_geom), never of the device, so the bits are too.  No
// floating-point atomics; per-thread fp32 partial sums of r^2, a fixed-order tree per workgroup, doubles from there on.  A tile is owned by
// one workgroup and all of it is read before any of it is written: g_img may alias y_hat.
#pragma once
#include "common.h"
#include "norm_elem.h"

// where a kernel takes sqrt(abar_t) and sqrt(1 - abar_t) from: the sampler's 8-float rows and device step counter (st != null), or by value
struct GuideCoefSrc { const float* coef; const SamplerState* st; int n_steps; float a, s; int pred; };
__device__ __forceinline__ int guide_coef_load(const GuideCoefSrc& g, float& a, float& s, float& inv_a) {
#pragma clang fp contract(off)
    int k = 0;
    a = g.a; s = g.s; inv_a = 1.0f / g.a;
    if (g.st) {
        k = g.st->k;
        const float* c = g.coef + (size_t)(k < g.n_steps ? k : g.n_steps - 1) * 8;
        inv_a = c[0]; s = c[1]; a = c[6];
    }
    return k;
}

// z0 := x0_hat(x, m) * inv_sf over n elements
__global__ __launch_bounds__(256) void guidance_x0_kernel(const float* __restrict__ x, const float* __restrict__ m, float* __restrict__ z0,
                                                          const GuideCoefSrc g, float inv_sf, long n) {
#pragma clang fp contract(off)
    float a, s, inv_a;
    guide_coef_load(g, a, s, inv_a);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float xv = x[i], mv = m[i];
        const float x0 = g.pred == PRED_EPSILON ? (xv - s * mv) * inv_a : g.pred == PRED_SAMPLE ? mv : a * xv - s * mv;
        z0[i] = x0 * inv_sf;
    }
}

// grad_out := c_m (dz * inv_sf), gx := c_x (dz * inv_sf) over n elements
__global__ __launch_bounds__(256) void guidance_chain_kernel(const float* __restrict__ dz, float* __restrict__ grad_out, float* __restrict__ gx,
                                                             const GuideCoefSrc g, float inv_sf, long n) {
#pragma clang fp contract(off)
    float a, s, inv_a;
    guide_coef_load(g, a, s, inv_a);
    float cx, cm;
    if (g.pred == PRED_EPSILON) { cx = inv_a; cm = -s * inv_a; }
    else if (g.pred == PRED_SAMPLE) { cx = 0.f; cm = 1.f; }
    else { cx = a; cm = -s; }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float d = dz[i] * inv_sf;
        grad_out[i] = cm * d; gx[i] = cx * d;
    }
}

enum { IMG_RES_STAGE = 4096,       // floats of LDS a tile's rows are staged through at a time
       IMG_RES_CHUNK = 4096 };     // image voxels a workgroup aims at
// the work split of image_residual_kernel, from the shape alone.  pool == 1: cw = 0, a chunk is IMG_RES_CHUNK consecutive voxels of the sample
struct ImageResGeom { int cw, nseg, tiles_per_chunk; long tiles, chunks; };
static inline ImageResGeom image_residual_geom(int C, int D, int H, int W, int pool) {
    ImageResGeom g{};
    if (pool == 1) { g.chunks = ((long)C * D * H * W + IMG_RES_CHUNK - 1) / IMG_RES_CHUNK; return g; }
    const int pw = W / pool;
    int cw = 1024 / pool; if (cw < 1) cw = 1; if (cw > 256) cw = 256; if (cw > pw) cw = pw;
    g.cw = cw; g.nseg = (pw + cw - 1) / cw;
    const long tile_vox = (long)pool * pool * pool * cw;
    g.tiles_per_chunk = tile_vox >= IMG_RES_CHUNK ? 1 : (int)(IMG_RES_CHUNK / tile_vox);
    g.tiles = (long)C * (D / pool) * (H / pool) * g.nseg;
    g.chunks = (g.tiles + g.tiles_per_chunk - 1) / g.tiles_per_chunk;
    return g;
}

struct ImageResParams {
    const float* y_hat;                              // the decoded prediction, fp32 [B][C][D][H][W]
    const float* target; int target_batch;           // y [1 or B][C][D/p][H/p][W/p]
    const float* weight; int weight_batch;           // w, the target's shape per sample, [1 or B]; null: 1
    float* g_img;                                    // [B][C][D][H][W]; may alias y_hat
    double* partials;                                // [B][chunks]
    int pool, C, D, H, W;
    ImageResGeom geom;
};

__global__ __launch_bounds__(256) void image_residual_kernel(const ImageResParams p) {
#pragma clang fp contract(off)
    __shared__ float stage[IMG_RES_STAGE];
    __shared__ float rowsum[IMG_RES_STAGE];
    __shared__ float gcell[256];
    __shared__ float red[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long chunk = blockIdx.x;
    const int pl = p.pool, pd = p.D / pl, ph = p.H / pl, pw = p.W / pl;
    const long cells = (long)p.C * pd * ph * pw, dhw = (long)p.D * p.H * p.W, per = (long)p.C * dhw;
    const float* yb = p.y_hat + (size_t)b * per;
    float* gb = p.g_img + (size_t)b * per;
    const float* tb = p.target + (p.target_batch > 1 ? (size_t)b * cells : 0);
    const float* wb = p.weight ? p.weight + (p.weight_batch > 1 ? (size_t)b * cells : 0) : nullptr;
    float part = 0.f;
    if (pl == 1) {                                      // voxel identity: a contiguous run, lane after lane
        const long i0 = chunk * IMG_RES_CHUNK, i1 = i0 + IMG_RES_CHUNK < per ? i0 + IMG_RES_CHUNK : per;
        for (long i = i0 + tid; i < i1; i += 256) {
            const float w = wb ? wb[i] : 1.f;
            const float res = w * (yb[i] - tb[i]);
            part += res * res;
            gb[i] = w * res;
        }
    } else {
        const int cw = p.geom.cw, nseg = p.geom.nseg, p2 = pl * pl;
        int R = IMG_RES_STAGE / (cw * pl); if (R > p2) R = p2;          // rows staged at a time
        const float inv_p3 = 1.0f / (float)(p2 * pl);
        const long t0 = chunk * p.geom.tiles_per_chunk, t1 = t0 + p.geom.tiles_per_chunk < p.geom.tiles ? t0 + p.geom.tiles_per_chunk : p.geom.tiles;
        for (long tile = t0; tile < t1; ++tile) {
            const int seg = (int)(tile % nseg); long r = tile / nseg;
            const int qh = (int)(r % ph); r /= ph; const int qd = (int)(r % pd); const int c = (int)(r / pd);
            const int cwn = seg * cw + cw <= pw ? cw : pw - seg * cw;      // cubes of this tile, floats of a row segment
            const int segf = cwn * pl;
            const long base = (long)c * dhw + ((long)qd * pl * p.H + (long)qh * pl) * p.W + (long)seg * cw * pl;
            float acc = 0.f;
            for (int r0 = 0; r0 < p2; r0 += R) {
                const int nr = r0 + R <= p2 ? R : p2 - r0;
                for (int i = tid; i < nr * segf; i += 256) {
                    const int rr = i / segf, col = i - rr * segf, row = r0 + rr, dz = row / pl, dy = row - dz * pl;
                    stage[i] = yb[base + ((long)dz * p.H + dy) * p.W + col];
                }
                __syncthreads();
                for (int i = tid; i < nr * cwn; i += 256) {               // one (row, cube) pair: pool floats in order
                    const int rr = i / cwn, t = i - rr * cwn;
                    const float* sp = stage + rr * segf + t * pl;
                    float s = 0.f;
                    for (int dx = 0; dx < pl; ++dx) s += sp[dx];
                    rowsum[i] = s;
                }
                __syncthreads();
                if (tid < cwn) for (int rr = 0; rr < nr; ++rr) acc += rowsum[rr * cwn + tid];      // rows in order
            }
            if (tid < cwn) {
                const long q = (((long)c * pd + qd) * ph + qh) * pw + (long)seg * cw + tid;
                const float w = wb ? wb[q] : 1.f;
                const float res = w * (acc * inv_p3 - tb[q]);
                part += res * res;
                gcell[tid] = inv_p3 * (w * res);
            }
            __syncthreads();
            for (int i = tid; i < p2 * segf; i += 256) {
                const int row = i / segf, col = i - row * segf, dz = row / pl, dy = row - dz * pl;
                gb[base + ((long)dz * p.H + dy) * p.W + col] = gcell[col / pl];
            }
            __syncthreads();                              // gcell and the staging buffers are the next tile's
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                  // fixed order: the same inputs give the same bits
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) p.partials[(size_t)b * p.geom.chunks + chunk] = (double)red[0];
}

// norm2[b] := sum of sample b's partials in index order (double), norm_tab[k][b] := |r_b| at the sampler's step k (st null: row 0)
__global__ __launch_bounds__(64) void image_residual_fold_kernel(const double* __restrict__ partials, long chunks, float* __restrict__ norm2,
                                                                 float* __restrict__ norm_tab, const SamplerState* st, int n_steps, int B) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    const double* pb = partials + (size_t)b * chunks;
    double sum = 0.0;
    for (long i = 0; i < chunks; ++i) sum += pb[i];
    norm2[b] = (float)sum;
    const int k = st ? st->k : 0;
    if (norm_tab && k < n_steps) norm_tab[(size_t)k * B + b] = (float)sqrt(sum);
}
