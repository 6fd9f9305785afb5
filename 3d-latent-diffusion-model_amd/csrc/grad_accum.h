// Gradient accumulation over micro-batches: one streaming fp32 pass over a range of the flat gradient buffer,
//   assign:  acc[i] = g[i] * s            (nothing of acc is read: it needs no zeroing, stale contents cannot leak in)
//   add:     acc[i] = acc[i] + g[i] * s
// run by the backward plans at every OP_BUCKET over the tail range that has just become final (ldm_model_set_grad_accum), and on its own by
// ldm_op_grad_accumulate.  One writer per element, no atomics; the product is rounded before the sum (contraction off), so the result is
// the same bits as the two fp32 operations written out, and NaN / inf travel by ordinary arithmetic.
//
// A range starts anywhere in the buffer (bucket boundaries fall on parameter boundaries), but acc + first and g + first share their
// misalignment: `head` scalar elements reach the first 16-byte boundary, `nvec` float4 follow, and up to three scalar elements finish.  The
// launcher passes head = n for a pointer pair whose misalignments differ (the op entry only): everything scalar.
#pragma once
#include "common.h"

// Plain loads of g: non-temporal ones (neither buffer is read again before ~1.5 GB of other traffic at full size) were measured inside
// backward and lost on the add pass, which a window runs K - 1 times
template <bool ASSIGN>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ acc, const float* __restrict__ g, long head, long nvec, long tail, float s) {
#pragma clang fp contract(off)
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    f32x4* a4 = reinterpret_cast<f32x4*>(acc + head);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + head);
    for (long i = tid; i < nvec; i += stride) {
        const f32x4 p = g4[i] * s;
        if (ASSIGN) a4[i] = p;
        else a4[i] = a4[i] + p;
    }
    for (long e = tid; e < head + tail; e += stride) {       // the scalar ends: at most 3 + 3 elements (or all n of an unaligned pair)
        const long i = e < head ? e : 4 * nvec + e;
        const float p = g[i] * s;
        if (ASSIGN) acc[i] = p;
        else acc[i] = acc[i] + p;
    }
}
