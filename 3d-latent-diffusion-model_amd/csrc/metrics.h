// Image-quality metrics of a denoised volume against its target (ldm_op_image_metrics): 3-D SSIM with a separable window, and the
// error sums behind PSNR / MSE / MAE / NRMSE, in ONE pass over a pair of fp32 volumes [B, C, D, H, W] (W contiguous, the other
// strides the caller's: a cropped view of a padded buffer is scored in place).
//
// Shape.  A 256-thread workgroup owns an MT_TH x MT_TW (16 x 32) tile of the valid SSIM map and a run of output planes, and marches
// along D.  Per input plane it loads the haloed (16 + win - 1) x (32 + win - 1) tile of x and y into LDS (pivot subtracted), filters
// the five products x, y, xx, yy, xy along W (LDS -> LDS) and then along H (LDS -> registers); every thread holds two output pixels
// of the tile.  The D direction is a shift register per pixel and product: A[j] is the partial sum of the output plane that started
// j planes ago, A[j] <- A[j-1] + w[j] * v, and A[win-1] leaves as a finished voxel of the map.  Indices are compile-time constants
// (WIN is a template argument), so the 2 x 5 x win partial sums live in VGPRs.  Every input plane is read once per workgroup.
//
// Cancellation.  var = E[x^2] - mu^2 on raw fp32 values loses what a nearly flat image (PET background, uniform uptake) has to
// offer: with values near 0.9 the products carry 6e-8 of rounding against variances of 1e-7.  Variances and the covariance are
// shift invariant, so each workgroup subtracts a pivot (the mean of its tile's first input plane, one per volume of the pair) before
// it forms products and adds it back to the two means only.
//
// Error sums.  The same loads feed sum (x-y)^2, sum |x-y|, sum y^2, min y, max y, in double.  The haloed tiles overlap, so each input
// voxel has one OWNER: the workgroup whose tile origin box [h0, h0 + 16) x [w0, w0 + 32) x [d0, d0 + planes) holds it; the last tile /
// run of each axis also owns the trailing win - 1 voxels.
//
// Reduction.  Each workgroup folds its threads' doubles over a fixed LDS tree and writes one MetricsPartial; metrics_finalize_kernel
// (one workgroup per batch element) folds the partials in index order over the same tree.  No atomics: the same inputs give the same
// bits.
#define MT_TH 16
#define MT_TW 32
#define MT_THREADS 256
#define MT_MAXWIN 11

struct MetricsPartial { double ssim, se, ae, yy, ymin, ymax, pad0, pad1; };

struct MetricsParams {
    const float* x; const float* y;
    long xs[4], ys[4];                 // element strides of B, C, D, H
    int B, C, D, H, W;
    int Do, Ho, Wo;                    // the valid map: D - win + 1, ...
    int tiles_h, tiles_w, nchunk, planes;     // output planes per workgroup = planes (the last run takes what is left)
    float w[MT_MAXWIN];
    float c1, c2;
    float* map;                        // optional [B][C][Do][Ho][Wo]
    MetricsPartial* partial;           // [B][C][nchunk][tiles_h][tiles_w]
};

// fixed-order fold of one double per thread: sum (op 0), min (1) or max (2); result valid in thread 0
__device__ __forceinline__ double metrics_block_fold(double v, double* red, int op) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double a = red[tid], b = red[tid + s];
            red[tid] = op == 0 ? a + b : op == 1 ? fmin(a, b) : fmax(a, b);
        }
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ float ssim_voxel(float mxp, float myp, float exx, float eyy, float exy, float px, float py, float c1, float c2) {
#pragma clang fp contract(off)            // x == y must give the same bits above and below the division: exactly 1
    const float sxx = __fmaf_rn(-mxp, mxp, exx), syy = __fmaf_rn(-myp, myp, eyy), sxy = __fmaf_rn(-mxp, myp, exy);
    const float mx = mxp + px, my = myp + py;
    const float num = (2.f * (mx * my) + c1) * (2.f * sxy + c2);
    const float den = ((mx * mx + my * my) + c1) * ((sxx + syy) + c2);
    return num / den;
}

template <int WIN>
__global__ __launch_bounds__(MT_THREADS) void image_metrics_kernel(const MetricsParams p) {
    constexpr int IH = MT_TH + WIN - 1, IW = MT_TW + WIN - 1;
    __shared__ float sx[IH * IW], sy[IH * IW];
    __shared__ float st[5][IH * MT_TW];
    __shared__ double red[MT_THREADS];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int tw = bid % p.tiles_w; bid /= p.tiles_w;
    const int th = bid % p.tiles_h; bid /= p.tiles_h;
    const int ck = bid % p.nchunk; bid /= p.nchunk;
    const int c = bid % p.C, b = bid / p.C;
    const int h0 = th * MT_TH, w0 = tw * MT_TW, d0 = ck * p.planes;
    const int nout = min(p.planes, p.Do - d0);                       // output planes of this run
    const int din_end = d0 + nout + WIN - 1;                         // <= D
    const bool last_h = th == p.tiles_h - 1, last_w = tw == p.tiles_w - 1, last_d = ck == p.nchunk - 1;
    const float* xb = p.x + b * p.xs[0] + c * p.xs[1];
    const float* yb = p.y + b * p.ys[0] + c * p.ys[1];

    // pivots: mean of the tile's first input plane (in-bounds part)
    float px, py;
    {
        float ax = 0.f, ay = 0.f;
        for (int i = tid; i < IH * IW; i += MT_THREADS) {
            const int r = i / IW, q = i - r * IW, h = h0 + r, w = w0 + q;
            if (h < p.H && w < p.W) {
                ax += xb[d0 * p.xs[2] + h * p.xs[3] + w];
                ay += yb[d0 * p.ys[2] + h * p.ys[3] + w];
            }
        }
        const int cnt = min(IH, p.H - h0) * min(IW, p.W - w0);
        px = (float)(metrics_block_fold((double)ax, red, 0) / cnt);
        py = (float)(metrics_block_fold((double)ay, red, 0) / cnt);
    }

    double se = 0.0, ae = 0.0, yy = 0.0, ssum = 0.0;
    float ymin = INFINITY, ymax = -INFINITY;
    float A[2][5][WIN];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < WIN; ++j) A[o][q][j] = 0.f;
    const int tx = tid % MT_TW, ty = tid / MT_TW;                    // output pixels (ty, tx) and (ty + 8, tx) of the tile
    const long map_bc = ((long)b * p.C + c) * p.Do;

    for (int d = d0; d < din_end; ++d) {
        const bool own_d = d < d0 + p.planes || last_d;
        const float* xp = xb + d * p.xs[2];
        const float* yp = yb + d * p.ys[2];
        __syncthreads();                                             // the previous plane's W filter has read sx / sy
        for (int i = tid; i < IH * IW; i += MT_THREADS) {
            const int r = i / IW, q = i - r * IW, h = h0 + r, w = w0 + q;
            float vx = 0.f, vy = 0.f;
            if (h < p.H && w < p.W) {
                const float gx = xp[h * p.xs[3] + w], gy = yp[h * p.ys[3] + w];
                vx = gx - px; vy = gy - py;
                if (own_d && (r < MT_TH || last_h) && (q < MT_TW || last_w)) {
                    const double df = (double)gx - (double)gy;
                    se = fma(df, df, se); ae += fabs(df); yy = fma((double)gy, (double)gy, yy);
                    ymin = fminf(ymin, gy); ymax = fmaxf(ymax, gy);
                }
            }
            sx[i] = vx; sy[i] = vy;
        }
        __syncthreads();
        for (int i = tid; i < IH * MT_TW; i += MT_THREADS) {         // along W: five products per (row, output column)
            const int r = i / MT_TW, q = i - r * MT_TW;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float a = sx[r * IW + q + k], e = sy[r * IW + q + k], wk = p.w[k];
                m0 = __fmaf_rn(wk, a, m0); m1 = __fmaf_rn(wk, e, m1);
                m2 = __fmaf_rn(wk, a * a, m2); m3 = __fmaf_rn(wk, e * e, m3); m4 = __fmaf_rn(wk, a * e, m4);
            }
            st[0][i] = m0; st[1][i] = m1; st[2][i] = m2; st[3][i] = m3; st[4][i] = m4;
        }
        __syncthreads();
        const bool emit = d - d0 >= WIN - 1;
        const int dout = d - (WIN - 1);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int r0 = ty + o * (MT_TH / 2);
            float v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {                            // along H
                float m = 0.f;
#pragma unroll
                for (int k = 0; k < WIN; ++k) m = __fmaf_rn(p.w[k], st[q][(r0 + k) * MT_TW + tx], m);
                v[q] = m;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) {                            // along D: the shift register
#pragma unroll
                for (int j = WIN - 1; j > 0; --j) A[o][q][j] = __fmaf_rn(p.w[j], v[q], A[o][q][j - 1]);
                A[o][q][0] = p.w[0] * v[q];
            }
            const int ho = h0 + r0, wo = w0 + tx;
            if (emit && ho < p.Ho && wo < p.Wo) {
                const float s = ssim_voxel(A[o][0][WIN - 1], A[o][1][WIN - 1], A[o][2][WIN - 1], A[o][3][WIN - 1], A[o][4][WIN - 1],
                                           px, py, p.c1, p.c2);
                ssum += (double)s;
                if (p.map) p.map[((map_bc + dout) * p.Ho + ho) * p.Wo + wo] = s;
            }
        }
    }
    const double f0 = metrics_block_fold(ssum, red, 0), f1 = metrics_block_fold(se, red, 0), f2 = metrics_block_fold(ae, red, 0),
                 f3 = metrics_block_fold(yy, red, 0), f4 = metrics_block_fold((double)ymin, red, 1), f5 = metrics_block_fold((double)ymax, red, 2);
    if (tid == 0) {
        MetricsPartial r; r.ssim = f0; r.se = f1; r.ae = f2; r.yy = f3; r.ymin = f4; r.ymax = f5; r.pad0 = 0.0; r.pad1 = 0.0;
        p.partial[blockIdx.x] = r;
    }
}

// out[b][8] = ssim, psnr, mse, mae, nrmse, min(y), max(y), 0; the batch element's partials folded in index order
__global__ __launch_bounds__(MT_THREADS) void metrics_finalize_kernel(const MetricsPartial* __restrict__ partial, int per_batch, double n_map,
                                                                      double n_vox, float max_val, float* __restrict__ out) {
    __shared__ double red[MT_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const MetricsPartial* pb = partial + (long)b * per_batch;
    double s = 0.0, se = 0.0, ae = 0.0, yy = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int i = tid; i < per_batch; i += MT_THREADS) {
        const MetricsPartial r = pb[i];
        s += r.ssim; se += r.se; ae += r.ae; yy += r.yy; lo = fmin(lo, r.ymin); hi = fmax(hi, r.ymax);
    }
    s = metrics_block_fold(s, red, 0); se = metrics_block_fold(se, red, 0); ae = metrics_block_fold(ae, red, 0);
    yy = metrics_block_fold(yy, red, 0); lo = metrics_block_fold(lo, red, 1); hi = metrics_block_fold(hi, red, 2);
    if (tid == 0) {
        const double mse = se / n_vox;
        float* o = out + (long)b * 8;
        o[0] = (float)(s / n_map);
        o[1] = (float)(20.0 * log10((double)max_val) - 10.0 * log10(mse));        // mse == 0: +inf, as MONAI's 10 log10
        o[2] = (float)mse;
        o[3] = (float)(ae / n_vox);
        o[4] = (float)sqrt(se / yy);
        o[5] = (float)lo; o[6] = (float)hi; o[7] = 0.f;
    }
}

struct MetricsPlan { int tiles_h, tiles_w, nchunk, planes; long groups; };

// D is cut into runs of output planes so that a whole scan fills the chip (about two workgroups per CU); a run re-reads win - 1
// planes of halo, so runs are no shorter than 8 planes.
static MetricsPlan metrics_plan(int B, int C, int D, int H, int W, int win) {
    MetricsPlan m;
    const int Do = D - win + 1, Ho = H - win + 1, Wo = W - win + 1;
    m.tiles_h = (Ho + MT_TH - 1) / MT_TH; m.tiles_w = (Wo + MT_TW - 1) / MT_TW;
    const long flat = (long)B * C * m.tiles_h * m.tiles_w;
    long want = (512 + flat - 1) / flat;
    const int max_runs = (Do + 7) / 8;
    if (want > max_runs) want = max_runs;
    if (want < 1) want = 1;
    m.planes = (int)((Do + want - 1) / want);
    m.nchunk = (Do + m.planes - 1) / m.planes;
    m.groups = flat * m.nchunk;
    return m;
}

static void launch_image_metrics(const MetricsParams& p, int win, long groups, hipStream_t s) {
    const dim3 g((unsigned)groups), t(MT_THREADS);
    switch (win) {
        case 3: hipLaunchKernelGGL(image_metrics_kernel<3>, g, t, 0, s, p); break;
        case 5: hipLaunchKernelGGL(image_metrics_kernel<5>, g, t, 0, s, p); break;
        case 7: hipLaunchKernelGGL(image_metrics_kernel<7>, g, t, 0, s, p); break;
        case 9: hipLaunchKernelGGL(image_metrics_kernel<9>, g, t, 0, s, p); break;
        default: hipLaunchKernelGGL(image_metrics_kernel<11>, g, t, 0, s, p); break;
    }
}
