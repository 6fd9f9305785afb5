// Sliding-window latent sampling (ldm_window_*, ldm_unet_denoise_step_windows): a full latent [C, D, H, W] is cut into a grid of
// overlapping windows [nW, C, rd, rh, rw] of the size the UNet was trained on, the UNet runs on the batch of windows, and the windows'
// eps predictions are blended back with a separable importance map before one scheduler step on the whole latent.
//
// The grid (host-built, sliding.py): per axis a the window starts s_a[0..n_a) (ascending, first 0, last dim_a - roi_a), the
// normalised per-axis weight table t_a[i][0..roi_a) and the cover table cover_a[p] = {first window covering p, count}.  Window
// (i, j, k) has flat index (i * n_h + j) * n_w + k.  The weight of window (i, j, k) at voxel p is t_d[i][.] * t_h[j][.] * t_w[k][.]
// and these sum to 1 over the windows covering p.
//
// No atomics on data: every output element has exactly one writer, and a voxel sums its windows in ascending window order, so
// every result is bitwise reproducible.  The only atomic is the sampler's block-completion counter (sampler_advance), as in
// sampler_step_kernel.
struct WinGeom {
    int dim[3], roi[3], n[3];
    const int* start[3];            // [n_a]
    const float* tab[3];            // [n_a][roi_a]
    const int2* cover[3];           // [dim_a] {first, count}
};

// blend of channel c at voxel (pd, ph, pw): sum over the covering windows, ascending, of w * src[win][c][local]
__device__ __forceinline__ float window_blend_at(const WinGeom& g, const float* __restrict__ src, int C, int c, int pd, int ph, int pw) {
#pragma clang fp contract(off)                                  // the same bits in window_blend_kernel and window_blend_step_kernel
    const int2 cd = g.cover[0][pd], ch = g.cover[1][ph], cw = g.cover[2][pw];
    const long r3 = (long)g.roi[0] * g.roi[1] * g.roi[2];
    float acc = 0.f;
    bool first = true;
    for (int a = cd.x; a < cd.x + cd.y; ++a) {
        const int zd = pd - g.start[0][a];
        const float td = g.tab[0][(long)a * g.roi[0] + zd];
        for (int b = ch.x; b < ch.x + ch.y; ++b) {
            const int zh = ph - g.start[1][b];
            const float tdh = td * g.tab[1][(long)b * g.roi[1] + zh];
            for (int e = cw.x; e < cw.x + cw.y; ++e) {
                const int zw = pw - g.start[2][e];
                const float w = tdh * g.tab[2][(long)e * g.roi[2] + zw];
                const long win = ((long)a * g.n[1] + b) * g.n[2] + e;
                const float v = src[(win * C + c) * r3 + ((long)zd * g.roi[1] + zh) * g.roi[2] + zw];
                acc = first ? w * v : __fmaf_rn(w, v, acc);      // one window of weight 1: v exactly
                first = false;
            }
        }
    }
    return acc;
}

// full volume [C, D, H, W] -> windows [nW, C, rd, rh, rw]
__global__ __launch_bounds__(256) void window_gather_kernel(const WinGeom g, const float* __restrict__ src, float* __restrict__ dst, int C) {
    const long r3 = (long)g.roi[0] * g.roi[1] * g.roi[2];
    const long total = (long)g.n[0] * g.n[1] * g.n[2] * C * r3;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        long r = o;
        const int zw = (int)(r % g.roi[2]); r /= g.roi[2];
        const int zh = (int)(r % g.roi[1]); r /= g.roi[1];
        const int zd = (int)(r % g.roi[0]); r /= g.roi[0];
        const int c = (int)(r % C); r /= C;
        const int e = (int)(r % g.n[2]); r /= g.n[2];
        const int b = (int)(r % g.n[1]); const int a = (int)(r / g.n[1]);
        const int pd = g.start[0][a] + zd, ph = g.start[1][b] + zh, pw = g.start[2][e] + zw;
        dst[o] = src[(((long)c * g.dim[0] + pd) * g.dim[1] + ph) * g.dim[2] + pw];
    }
}

// windows [nW, C, r^3] -> full volume [C, D, H, W] (the blend alone: host-driven sampling loop, tests)
__global__ __launch_bounds__(256) void window_blend_kernel(const WinGeom g, const float* __restrict__ src, float* __restrict__ dst, int C) {
    const long vox = (long)g.dim[0] * g.dim[1] * g.dim[2], total = vox * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long r = i;
        const int pw = (int)(r % g.dim[2]); r /= g.dim[2];
        const int ph = (int)(r % g.dim[1]); r /= g.dim[1];
        const int pd = (int)(r % g.dim[0]); const int c = (int)(r / g.dim[0]);
        dst[i] = window_blend_at(g, src, C, c, pd, ph, pw);
    }
}

// every window slot of xw [nW, C, r^3] that covers voxel (pd, ph, pw) of channel c := v
__device__ __forceinline__ void window_write_back(const WinGeom& g, float* __restrict__ xw, int C, int c, int pd, int ph, int pw, float v) {
    const long r3 = (long)g.roi[0] * g.roi[1] * g.roi[2];
    const int2 cd = g.cover[0][pd], chh = g.cover[1][ph], cw = g.cover[2][pw];
    for (int a = cd.x; a < cd.x + cd.y; ++a) {
        const long od = (long)(pd - g.start[0][a]) * g.roi[1];
        for (int b = chh.x; b < chh.x + chh.y; ++b) {
            const long oh = (od + (ph - g.start[1][b])) * g.roi[2];
            for (int e = cw.x; e < cw.x + cw.y; ++e) {
                const long win = ((long)a * g.n[1] + b) * g.n[2] + e;
                xw[(win * C + c) * r3 + oh + (pw - g.start[2][e])] = v;
            }
        }
    }
}

// One windowed denoising step after the UNet has run on every window: for every element i of the full latent x [C, D, H, W]
//   m = blend(p.m)(i);  x[i] := the step rule's update of (x[i], m, z);  every window slot of xw that covers i := x[i]
// as the source of the one step loop (norm_elem.h sampler_step_loop), so every scheduler family runs on the full latent exactly as
// sampler_step_kernel runs it: the noise z of element i is the sampler's draw for (flat index quad i / 4, step k) whatever the window
// grid, a PNDM history holds blended full-latent outputs, and the last block advances the step counter and writes tbuf[0..B).
// The model output is blended before the rule converts it: every rule is affine in m with coefficients that are the same at every
// element of a step (DDPM / DDIM per prediction type, PNDM in all its model outputs, the flow's Euler step, DPM-Solver++'s conversion
// to x0_hat), so the update commutes with the blend's convex combination and runs once per element; a DPM-Solver++ state therefore
// holds the x0_hat of the blended full-latent output, converted and clamped once per element.
struct StepWindows {
    const WinGeom& g;
    template <class Step> __device__ __forceinline__ void operator()(const StepParams& p, long i, Step&& step) const {
        long r = i;
        const int pw = (int)(r % g.dim[2]); r /= g.dim[2];
        const int ph = (int)(r % g.dim[1]); r /= g.dim[1];
        const int pd = (int)(r % g.dim[0]); const int ch = (int)(r / g.dim[0]);
        const float xn = step(window_blend_at(g, p.m, p.C, ch, pd, ph, pw));
        window_write_back(g, p.xw, p.C, ch, pd, ph, pw, xn);
    }
};
template <int PRED, int FAMILY = STEP_DDPM>
__global__ __launch_bounds__(256) void window_blend_step_kernel(const WinGeom g, const StepParams p) {   // p.n = C * dim[0] * dim[1] * dim[2]
    sampler_step_loop<StepRule<PRED, FAMILY>>(p, StepWindows{g});
}
// the same for a DPM-Solver++ sampler, under a name of its own (see dpm_sampler_step_kernel)
template <int PRED>
__global__ __launch_bounds__(256) void dpm_window_step_kernel(const WinGeom g, const StepParams p) {
    sampler_step_loop<StepRule<PRED, STEP_DPM>>(p, StepWindows{g});
}
